// gsr_mesh_bake.hip -- the colour half of the mesh <-> Gaussians loop: the per-view body of gaustudio/scripts/texture_mesh.py
// (per-vertex colours baked from posed photographs, :108-141) and MeshInitializer.build_model
// (gaustudio/pipelines/initializers/mesh.py:20-250: n flat Gaussians per triangle), for a mesh that stays in HBM.
//
// Contract, float32 throughout, no contraction (Makefile: -ffp-contract=off; the only fused multiply-adds
// are the explicit fmaf of the seeds' norm3f / cross3f), correctly rounded divide / sqrt:
//   * bake_select, one lane per face.  For a face with visible[f] != 0: n = (v1 - v0) x (v2 - v0) (the cross product of s15),
//     |n| = sqrt((n.x^2 + n.y^2) + n.z^2), cos = ((n.x / |n|) d.x + (n.y / |n|) d.y) + (n.z / |n|) d.z with d the normalised third
//     row of the world-to-camera rotation.  cos < -0.05f selects the face: its three vertices get stamp[v] = seq, a plain store
//     (every racing store writes the same value).  |n| = 0 gives cos = NaN, which selects nothing.
//   * bake_sample, one lane per vertex with stamp[v] == seq.  Camera coordinates as s15; the reference's flipped screen
//     position x = (fx (-x_c)) / z_c + cx (PyTorch3D after the RDF->LUF flip), g = 2 (x / (W - 1)) - 1, valid when both g lie
//     in [-1, 1]; grid_sample(bilinear, align_corners=False, reflection) of the image flipped in both axes, clamped to [0, 1]
//     ("reference").  "exact": the OpenCV pixel u = (fx x_c) / z_c + cx, valid when 0 <= u <= W and 0 <= v <= H, sampled at
//     column u - 0.5, row v - 0.5 of the image as it is.
//   * seeds, one lane per (face, k), k < n, n in {1, 3, 4, 6}: barycentric position / normal / colour, normal2rotation and
//     rotmat2quaternion operation for operation (their sign() quirks included; norms and the cross product with the explicit
//     fused multiply-adds of torch's CPU kernels, see norm3f), scale log(2 s + 1e-7) of s = min edge x radius.
//     The two logarithms are float(log(double(x))): correctly rounded in effect, so that a float32 model reproduces them.
//
// MI355X: all three are gather-bound stream kernels -- 256-thread blocks, one work item per lane, no LDS, the per-view matrices
// passed by value (they arrive through scalar loads), a grid-tail guard, plain stores.  No atomics except the seeds' error flag.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsrast.h"
#include "gsr_ws.h"

namespace {

struct View {
	float r[12];            // row-major [R | t] of the world-to-camera matrix
	float fx, fy, cx, cy;
	float d[3];             // the viewing axis in world space: the third row of R, normalised
	int W, H;
};

__device__ __forceinline__ float3 cross3(float3 u, float3 v)
{
	return make_float3(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
}
__device__ __forceinline__ float3 sub3(float3 u, float3 v) { return make_float3(u.x - v.x, u.y - v.y, u.z - v.z); }
__device__ __forceinline__ float norm3(float3 u) { return sqrtf((u.x * u.x + u.y * u.y) + u.z * u.z); }
__device__ __forceinline__ float3 load3(const float* __restrict__ p, int i)
{
	return make_float3(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]);
}
__device__ __forceinline__ void store3(float* __restrict__ p, size_t i, float3 v)
{
	p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z;
}
// The seeds' norm and cross product, with the fused multiply-adds written out in the form torch's CPU kernels evaluate them
// (vector_norm: fma(z, z, fma(y, y, x x)); cross: fma(a, b, -(c d))): the quaternion of a rotation near 180 degrees divides by
// sqrt(1 + trace) ~ 0, which turns a 1-ulp difference here into thousands, and the reference's recorded values
// are reproduced only with its own roundings.
__device__ __forceinline__ float norm3f(float3 u) { return sqrtf(fmaf(u.z, u.z, fmaf(u.y, u.y, u.x * u.x))); }
__device__ __forceinline__ float3 cross3f(float3 u, float3 v)
{
	return make_float3(fmaf(u.y, v.z, -(u.z * v.y)), fmaf(u.z, v.x, -(u.x * v.z)), fmaf(u.x, v.y, -(u.y * v.x)));
}
// F.normalize: x / max(|x|, 1e-12)
__device__ __forceinline__ float3 normalize3(float3 u)
{
	const float len = norm3f(u);
	const float d = len < 1e-12f ? 1e-12f : len;      // clamp_min: a NaN length stays NaN
	return make_float3(u.x / d, u.y / d, u.z / d);
}
// torch.sign: -1, 0 or 1; 0 for NaN
__device__ __forceinline__ float sign1(float x) { return (float)((0.0f < x) - (x < 0.0f)); }
// torch.min over a row: NaN wins
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b < a ? b : a)); }

// ------------------------------------------------------------------------------------------------------ select
__global__ void __launch_bounds__(256) bake_select(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                   const unsigned char* __restrict__ visible, View vw, int seq,
                                                   int* __restrict__ stamp, float* __restrict__ cos_out)
{
	const int f = blockIdx.x * 256 + threadIdx.x;
	if (f >= F) return;
	float c = NAN;
	if (visible[f]) {
		const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
		if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
			const float3 p0 = load3(verts, i0), p1 = load3(verts, i1), p2 = load3(verts, i2);
			const float3 n = cross3(sub3(p1, p0), sub3(p2, p0));
			const float len = norm3(n);
			c = ((n.x / len) * vw.d[0] + (n.y / len) * vw.d[1]) + (n.z / len) * vw.d[2];
			if (c < -0.05f) {
				stamp[i0] = seq;
				stamp[i1] = seq;
				stamp[i2] = seq;
			}
		}
	}
	if (cos_out) cos_out[f] = c;
}

// ------------------------------------------------------------------------------------------------------ sample
// grid_sample's bilinear taps at (ix, iy), both already inside [0, W - 1] x [0, H - 1]; FLIP reads I[H - 1 - r, W - 1 - c]
template <bool FLIP>
__device__ __forceinline__ float3 bilinear(const float* __restrict__ img, int W, int H, float ix, float iy)
{
	const float fx0 = floorf(ix), fy0 = floorf(iy);
	const float fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
	const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
	const float w[4] = {(fx1 - ix) * (fy1 - iy), (ix - fx0) * (fy1 - iy), (fx1 - ix) * (iy - fy0), (ix - fx0) * (iy - fy0)};
	const int tx[4] = {x0, x1, x0, x1}, ty[4] = {y0, y0, y1, y1};
	float3 acc = make_float3(0.0f, 0.0f, 0.0f);
#pragma unroll
	for (int k = 0; k < 4; k++) {
		if (tx[k] < 0 || tx[k] >= W || ty[k] < 0 || ty[k] >= H) continue;    // x1 = W or y1 = H
		const int r = FLIP ? H - 1 - ty[k] : ty[k], c = FLIP ? W - 1 - tx[k] : tx[k];
		const float* t = img + 3 * ((size_t)r * W + c);
		acc.x = acc.x + t[0] * w[k];
		acc.y = acc.y + t[1] * w[k];
		acc.z = acc.z + t[2] * w[k];
	}
	return acc;
}
__device__ __forceinline__ float clip(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
__device__ __forceinline__ float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }   // NaN stays NaN

template <bool EXACT>
__global__ void __launch_bounds__(256) bake_sample(const float* __restrict__ verts, int V, const int* __restrict__ stamp, int seq,
                                                   View vw, const float* __restrict__ img, float* __restrict__ colors,
                                                   int* __restrict__ baked_by)
{
	const int v = blockIdx.x * 256 + threadIdx.x;
	if (v >= V) return;
	if (stamp[v] != seq) return;
	const float3 p = load3(verts, v);
	const float* r = vw.r;
	const float xc = ((r[0] * p.x + r[1] * p.y) + r[2] * p.z) + r[3];
	const float yc = ((r[4] * p.x + r[5] * p.y) + r[6] * p.z) + r[7];
	const float zc = ((r[8] * p.x + r[9] * p.y) + r[10] * p.z) + r[11];
	const float Wf = (float)vw.W, Hf = (float)vw.H;
	float ix, iy;
	if (EXACT) {
		const float u = (vw.fx * xc) / zc + vw.cx, w = (vw.fy * yc) / zc + vw.cy;
		if (!(u >= 0.0f && u <= Wf && w >= 0.0f && w <= Hf)) return;
		ix = u - 0.5f;
		iy = w - 0.5f;
	} else {
		const float x = (vw.fx * (-xc)) / zc + vw.cx, y = (vw.fy * (-yc)) / zc + vw.cy;
		const float gx = 2.0f * (x / (Wf - 1.0f)) - 1.0f, gy = 2.0f * (y / (Hf - 1.0f)) - 1.0f;
		if (!(gx >= -1.0f && gx <= 1.0f && gy >= -1.0f && gy <= 1.0f)) return;      // NaN fails
		ix = ((gx + 1.0f) * Wf - 1.0f) / 2.0f;
		iy = ((gy + 1.0f) * Hf - 1.0f) / 2.0f;
	}
	ix = clip(ix, 0.0f, Wf - 1.0f);
	iy = clip(iy, 0.0f, Hf - 1.0f);
	const float3 c = bilinear<!EXACT>(img, vw.W, vw.H, ix, iy);
	store3(colors, (size_t)v, make_float3(clamp01(c.x), clamp01(c.y), clamp01(c.z)));
	baked_by[v] = seq;
}

// ------------------------------------------------------------------------------------------------------ seeds
struct SeedTable {
	float b[6][3];          // surface_triangle_bary_coords
	float radius;           // surface_triangle_circle_radius
	float log_eps;          // log(0 * 2 + 1e-7): the flat axis
	float c0;               // sh_utils.C0
	int n;
};

__device__ __forceinline__ float3 bary3(const float* b, float3 a0, float3 a1, float3 a2)
{
	return make_float3((b[0] * a0.x + b[1] * a1.x) + b[2] * a2.x, (b[0] * a0.y + b[1] * a1.y) + b[2] * a2.y,
	                   (b[0] * a0.z + b[1] * a1.z) + b[2] * a2.z);
}

// normal2rotation after its F.normalize (n is the normalised normal) and rotmat2quaternion, not normalised: q[4] = (w, x, y, z)
__device__ __forceinline__ void normal_quat(float3 n, float* __restrict__ q)
{
	const float dot = (1.0f * n.x + 0.0f * n.y) + 0.0f * n.z;
	float3 r0 = make_float3(1.0f - dot * n.x, 0.0f - dot * n.y, 0.0f - dot * n.z);
	const float s0 = sign1(r0.x);
	r0 = normalize3(make_float3(r0.x * s0, r0.y * s0, r0.z * s0));
	float3 r1 = cross3f(n, r0);
	const float s1 = sign1(r1.y) * sign1(n.z);
	r1 = make_float3(r1.x * s1, r1.y * s1, r1.z * s1);
	// R = [r0 | r1 | n] (columns)
	const float tr = ((r0.x + r1.y) + n.z) + 1e-6f;
	const float q0 = sqrtf(1.0f + tr) / 2.0f;
	const float q4 = 4.0f * q0;
	q[0] = q0;
	q[1] = (r1.z - n.y) / q4;
	q[2] = (n.x - r0.z) / q4;
	q[3] = (r0.y - r1.x) / q4;
}

__global__ void __launch_bounds__(256) mesh_seeds(const float* __restrict__ verts, const float* __restrict__ normals,
                                                  const float* __restrict__ vcolors, int V, const int* __restrict__ faces,
                                                  long long P, SeedTable tb, float* __restrict__ xyz, float* __restrict__ f_dc,
                                                  float* __restrict__ scale, float* __restrict__ rot, int* status)
{
	const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
	if (g >= P) return;
	const int f = (int)(g / tb.n), k = (int)(g - (long long)f * tb.n);
	const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
	if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
		atomicOr(status, 1);
		return;
	}
	const float* b = tb.b[k];
	const float3 p0 = load3(verts, i0), p1 = load3(verts, i1), p2 = load3(verts, i2);
	store3(xyz, (size_t)g, bary3(b, p0, p1, p2));

	// _compute_colors -> RGB2SH; rgb = 1 without vertex colours (create_from_attribute)
	float3 c = make_float3(1.0f, 1.0f, 1.0f);
	if (vcolors) c = bary3(b, load3(vcolors, i0), load3(vcolors, i1), load3(vcolors, i2));
	store3(f_dc, (size_t)g, make_float3((c.x - 0.5f) / tb.c0, (c.y - 0.5f) / tb.c0, (c.z - 0.5f) / tb.c0));

	// _compute_scales: min edge x radius on two axes, 0 on the third, log(2 s + 1e-7)
	const float e = min_nan(min_nan(norm3f(sub3(p0, p1)), norm3f(sub3(p1, p2))), norm3f(sub3(p2, p0)));
	float s = e * tb.radius;
	s = (s != s) ? s : fmaxf(s, 0.0f);
	const float ls = (float)log((double)(s * 2.0f + 1e-7f));
	store3(scale, (size_t)g, make_float3(ls, ls, tb.log_eps));

	// _compute_surface_normals (one F.normalize) -> normal2rotation (a second one)
	normal_quat(normalize3(normalize3(bary3(b, load3(normals, i0), load3(normals, i1), load3(normals, i2)))), rot + 4 * (size_t)g);
}

// ------------------------------------------------------------------------------------------------------ point seeds
// VanillaPointCloud.create_from_attribute (gaustudio/models/vanilla_sg.py:69-97), one lane per point.  An absent input is
// NULL: rgb -> 1; scale_in -> log(sqrt(dist2 + 1e-7)) on all three axes; rot_in -> normal2rotation(normals), or (1, 0, 0, 0)
// without normals; opacity_in -> the scalar.
__global__ void __launch_bounds__(256) point_seeds(const float* __restrict__ xyz, const float* __restrict__ rgb,
                                                   const float* __restrict__ dist2, const float* __restrict__ scale_in,
                                                   const float* __restrict__ rot_in, const float* __restrict__ normals,
                                                   const float* __restrict__ opacity_in, float opacity, float c0, int n,
                                                   float* __restrict__ xyz_out, float* __restrict__ f_dc, float* __restrict__ scale,
                                                   float* __restrict__ rot, float* __restrict__ opacity_out)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	store3(xyz_out, (size_t)i, load3(xyz, i));
	const float3 c = rgb ? load3(rgb, i) : make_float3(1.0f, 1.0f, 1.0f);
	store3(f_dc, (size_t)i, make_float3((c.x - 0.5f) / c0, (c.y - 0.5f) / c0, (c.z - 0.5f) / c0));
	if (scale_in) {
		store3(scale, (size_t)i, load3(scale_in, i));
	} else {
		const float ls = (float)log((double)sqrtf(dist2[i] + 1e-7f));
		store3(scale, (size_t)i, make_float3(ls, ls, ls));
	}
	float* q = rot + 4 * (size_t)i;
	if (rot_in) {
		for (int a = 0; a < 4; a++) q[a] = rot_in[4 * (size_t)i + a];
	} else if (normals) {
		normal_quat(normalize3(load3(normals, i)), q);
	} else {
		q[0] = 1.0f; q[1] = 0.0f; q[2] = 0.0f; q[3] = 0.0f;
	}
	opacity_out[i] = opacity_in ? opacity_in[i] : opacity;
}

// DepthInitializer's float16 cache file and uint8 colours (gaustudio/pipelines/initializers/depth.py:50-89) without the disk:
// one lane per pixel of one frame
__device__ __forceinline__ float half_round(float x) { return (float)(_Float16)x; }
__global__ void __launch_bounds__(256) depth_seed_pack(const float* __restrict__ points, const float* __restrict__ image,
                                                       const float* __restrict__ depth, int n, float focal,
                                                       float* __restrict__ xyz, float* __restrict__ rgb, float* __restrict__ scale)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const float3 p = load3(points, i), c = load3(image, i);
	store3(xyz, (size_t)i, make_float3(half_round(p.x), half_round(p.y), half_round(p.z)));
	float col[3] = {c.x, c.y, c.z};
	for (int a = 0; a < 3; a++)   // half(c) * 255 in half, truncated to uint8, / 255 in float32
		col[a] = (float)(unsigned char)(int)half_round(half_round(col[a]) * 255.0f) / 255.0f;
	store3(rgb, (size_t)i, make_float3(col[0], col[1], col[2]));
	const float s = half_round(depth[i] / focal);
	const float ls = half_round((float)log((double)s));   // numpy's float16 log: through float32
	store3(scale, (size_t)i, make_float3(ls, ls, ls));
}

// [R | t], K and the viewing axis of one view; false when a value is not finite, fx or fy is 0 or the axis has no length
bool make_view(const float* intrinsics, const float* extrinsics, int W, int H, View& vw)
{
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 4; c++) vw.r[4 * r + c] = extrinsics[4 * r + c];
	for (int k = 0; k < 12; k++)
		if (!isfinite(vw.r[k])) return false;
	vw.fx = vw.fy = 1.0f;
	vw.cx = vw.cy = 0.0f;
	if (intrinsics) {
		vw.fx = intrinsics[0]; vw.fy = intrinsics[4]; vw.cx = intrinsics[2]; vw.cy = intrinsics[5];
		if (!isfinite(vw.fx) || !isfinite(vw.fy) || !isfinite(vw.cx) || !isfinite(vw.cy) || vw.fx == 0.0f || vw.fy == 0.0f) return false;
	}
	const float a = vw.r[8], b = vw.r[9], c = vw.r[10];
	const float len = sqrtf((a * a + b * b) + c * c);
	if (!(len > 0.0f) || !isfinite(len)) return false;
	vw.d[0] = a / len; vw.d[1] = b / len; vw.d[2] = c / len;
	vw.W = W; vw.H = H;
	return true;
}

}  // namespace

extern "C" {

int gsr_mesh_bake_select(const float* verts, int num_verts, const int* faces, int num_faces, const unsigned char* visible,
                         const float extrinsics[16], int seq, int* stamp, float* cos_out, void* stream)
{
	if (num_verts < 0 || num_faces < 0 || seq < 0 || !extrinsics) return GSR_ERR_ARG;
	View vw;
	if (!make_view(nullptr, extrinsics, 0, 0, vw)) return GSR_ERR_ARG;
	if (num_faces == 0) return GSR_OK;
	if (!faces || !visible || num_verts == 0 || !verts || !stamp) return GSR_ERR_ARG;
	hipLaunchKernelGGL(bake_select, dim3(blocks(num_faces)), dim3(256), 0, (hipStream_t)stream, verts, num_verts, faces, num_faces,
	                   visible, vw, seq, stamp, cos_out);
	GSR_TRY(hipGetLastError());
	return GSR_OK;
}

int gsr_mesh_bake_sample(const float* verts, int num_verts, const int* stamp, int seq, const float intrinsics[9],
                         const float extrinsics[16], const float* image, int height, int width, int exact, float* colors,
                         int* baked_by, void* stream)
{
	if (num_verts < 0 || seq < 0 || !intrinsics || !extrinsics || height <= 0 || width <= 0 || height > 16384 || width > 16384 || !image)
		return GSR_ERR_ARG;
	View vw;
	if (!make_view(intrinsics, extrinsics, width, height, vw)) return GSR_ERR_ARG;
	if (num_verts == 0) return GSR_OK;
	if (!verts || !stamp || !colors || !baked_by) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	if (exact)
		hipLaunchKernelGGL(bake_sample<true>, dim3(blocks(num_verts)), dim3(256), 0, s, verts, num_verts, stamp, seq, vw, image, colors, baked_by);
	else
		hipLaunchKernelGGL(bake_sample<false>, dim3(blocks(num_verts)), dim3(256), 0, s, verts, num_verts, stamp, seq, vw, image, colors, baked_by);
	GSR_TRY(hipGetLastError());
	return GSR_OK;
}

int gsr_mesh_seeds(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* verts, const float* normals,
                   const float* vertex_colors, int num_verts, const int* faces, int num_faces, int n_per_triangle, float* xyz,
                   float* f_dc, float* scale, float* rot, void* stream)
{
	static const double B1[1][3] = {{1 / 3., 1 / 3., 1 / 3.}};
	static const double B3[3][3] = {{1 / 2., 1 / 4., 1 / 4.}, {1 / 4., 1 / 2., 1 / 4.}, {1 / 4., 1 / 4., 1 / 2.}};
	static const double B4[4][3] = {{1 / 3., 1 / 3., 1 / 3.}, {2 / 3., 1 / 6., 1 / 6.}, {1 / 6., 2 / 3., 1 / 6.}, {1 / 6., 1 / 6., 2 / 3.}};
	static const double B6[6][3] = {{2 / 3., 1 / 6., 1 / 6.}, {1 / 6., 2 / 3., 1 / 6.}, {1 / 6., 1 / 6., 2 / 3.},
	                                {1 / 6., 5 / 12., 5 / 12.}, {5 / 12., 1 / 6., 5 / 12.}, {5 / 12., 5 / 12., 1 / 6.}};
	const double (*B)[3];
	double radius;
	switch (n_per_triangle) {
	case 1: B = B1; radius = 1. / 2. / sqrt(3.); break;
	case 3: B = B3; radius = 1. / 2. / (sqrt(3.) + 1.); break;
	case 4: B = B4; radius = 1 / (4. * sqrt(3.)); break;
	case 6: B = B6; radius = 1 / (4. + 2. * sqrt(3.)); break;
	default: return GSR_ERR_ARG;
	}
	if (num_verts < 0 || num_faces < 0) return GSR_ERR_ARG;
	const long long P = (long long)num_faces * n_per_triangle;
	if (P >= (1LL << 31)) return GSR_ERR_ARG;
	if (P == 0) return GSR_OK;
	if (!faces || num_verts == 0 || !verts || !normals || !xyz || !f_dc || !scale || !rot) return GSR_ERR_ARG;
	SeedTable tb;
	for (int k = 0; k < 6; k++)
		for (int c = 0; c < 3; c++) tb.b[k][c] = k < n_per_triangle ? (float)B[k][c] : 0.0f;
	tb.radius = (float)radius;
	tb.log_eps = (float)log((double)(0.0f * 2.0f + 1e-7f));
	tb.c0 = (float)0.28209479177387814;
	tb.n = n_per_triangle;
	hipStream_t s = (hipStream_t)stream;
	int* status;
	if (!ws_carve(workspace_alloc, workspace_ctx, [&](Arena& ws) { status = ws.take<int>(1); })) return GSR_ERR_ALLOC;
	GSR_TRY(hipMemsetAsync(status, 0, sizeof(int), s));
	hipLaunchKernelGGL(mesh_seeds, dim3(blocks(P)), dim3(256), 0, s, verts, normals, vertex_colors, num_verts, faces, P, tb, xyz, f_dc,
	                   scale, rot, status);
	GSR_TRY(hipGetLastError());
	return read_status(status, s);
}

int gsr_point_seeds(const float* xyz, const float* rgb, const float* dist2, const float* scale_in, const float* rot_in,
                    const float* normals, const float* opacity_in, float opacity, int num_points, float* xyz_out, float* f_dc,
                    float* scale, float* rot, float* opacity_out, void* stream)
{
	if (num_points < 0 || (rot_in && normals)) return GSR_ERR_ARG;
	if (num_points == 0) return GSR_OK;
	if (!xyz || (!dist2 == !scale_in) || !xyz_out || !f_dc || !scale || !rot || !opacity_out) return GSR_ERR_ARG;
	hipLaunchKernelGGL(point_seeds, dim3(blocks(num_points)), dim3(256), 0, (hipStream_t)stream, xyz, rgb, dist2, scale_in, rot_in,
	                   normals, opacity_in, opacity, (float)0.28209479177387814, num_points, xyz_out, f_dc, scale, rot, opacity_out);
	GSR_TRY(hipGetLastError());
	return GSR_OK;
}

int gsr_depth_seed_pack(const float* points, const float* image, const float* depth, int num_pixels, float focal, float* xyz,
                        float* rgb, float* scale, void* stream)
{
	if (num_pixels < 0) return GSR_ERR_ARG;
	if (num_pixels == 0) return GSR_OK;
	if (!points || !image || !depth || !xyz || !rgb || !scale) return GSR_ERR_ARG;
	hipLaunchKernelGGL(depth_seed_pack, dim3(blocks(num_pixels)), dim3(256), 0, (hipStream_t)stream, points, image, depth, num_pixels,
	                   focal, xyz, rgb, scale);
	GSR_TRY(hipGetLastError());
	return GSR_OK;
}

}  // extern "C"
