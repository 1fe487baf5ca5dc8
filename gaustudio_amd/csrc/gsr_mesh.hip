// gsr_mesh.hip -- a forward-only, deterministic, watertight z-buffer rasterizer for triangle meshes and the helpers that
// gaustudio/scripts/render_mesh.py and texture_mesh.py take from PyTorch3D (MeshRasterizer with blur_radius = 0 and
// faces_per_pixel = 1, interpolate_face_attributes, Meshes.verts_normals_packed, get_visible_faces).
//
// Contract, in camera space (OpenCV axes):
//   * every vertex is transformed once, x_c = ((R00 x + R01 y) + R02 z) + t0 (same for y_c, z_c), no FMA;
//   * pixel (i, j) casts d = (((j + 0.5) - cx) / fx, ((i + 0.5) - cy) / fy, 1);
//   * face (a, b, c): e_a = b x c, e_b = c x a, e_c = a x b, each component formed in fp64 from the fp32 vertices (exact
//     products, one subtraction) and rounded to fp32 once; E_k = (e_k.x d.x + e_k.y d.y) + e_k.z in fp32; the ray covers
//     the face when all E_k >= 0 or all E_k <= 0 and S = (E_a + E_b) + E_c != 0; lambda_k = E_k / S,
//     z = (l_a z_a + l_b z_b) + l_c z_c; a hit counts when z_near < z < inf;
//   * a face hits only pixels of its rectangle: the fp64 projected extent of the face clipped against z = z_near (1 - 2^-12),
//     padded by one pixel, clamped to the image (face_setup; tests/mesh_raster_model.py pixel_rect).  The test is per
//     pixel, so the image is a function of the ray and the face alone, never of where the 16 x 16 tile grid falls;
//   * each pixel keeps the lexicographic minimum of (z, face id) over its hits.
// Watertight where the fp32 edge lines stay within the rectangle's one-pixel pad of the exact ones: the cross product
// u x v is computed as (u.y v.z - u.z v.y, ...); the fp64 products commute, the fp64 subtraction is antisymmetric (FMA
// contraction is off, Makefile: -ffp-contract=off) and rounding to fp32 is symmetric, so v x u is the exact negative of
// u x v, and so is every E computed from it.  Two faces sharing the edge (b, c) therefore see exactly opposite values of
// that edge's function on every ray: no ray passes between them, and a ray exactly on the edge (E = +-0) is covered by
// both (the inclusive test), the lower id winning the z tie.  The rectangle can take such a hit away only where the
// rounded edge function puts it more than a pixel outside the exact face: needles a few thousandths of a pixel wide,
// thousands of pixels off the optical axis (INTEGRATION.md s15 gives the figures).
//
// MI355X design:
//   * mesh_xform: one lane per vertex -> float4 camera-space positions.
//   * face_setup: one lane per face: index check, edge functions (3 float4 per face), the culls (non-finite vertex,
//     coincident vertices, wholly behind z_near, back face, off screen) and the pixel rectangle from the face clipped
//     against z = z_near in fp64, padded by one pixel (two packed words per face; its tiles are what the face is binned
//     to).  The sort key is a lower bound of every z the face can produce (min z_k less 2^-16 relative, at least z_near).
//   * binning: per-face tile counts, an int64 exclusive scan, (tile << 32 | key bits, face) pairs emitted in face order,
//     a stable LSD radix sort of the 64-bit keys (8-bit counting-sort passes) -> each tile's faces in (key, id) order.
//   * mesh_walk: one 16 x 16 workgroup per tile; faces are staged 256 at a time in LDS (records, key, id, rectangle); a
//     face counts for a pixel inside its rectangle that passes the sign test.  A pixel stops once its best z is
//     below the next face's key (no later face can reach it); a wave stops when a ballot says all its pixels have; the
//     workgroup stops loading batches when no pixel is left.  The result is a total-order minimum: independent of the
//     processing order, bit-identical from run to run, no atomics on it.
//   * interpolate / vertex normals / visible faces: one lane per pixel / per vertex (normals summed in ascending
//     (face, corner) order after a stable radix sort by vertex) / per pixel (plain byte stores of the value 1).
// No float atomics anywhere in this file; the only atomics are integer histogram counts in LDS and an error flag.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsrast.h"
#include "gsr_sort.h"

namespace {

constexpr int TILE = 16;
constexpr int MAX_DIM = 16384;          // width / height limit: at most 1024 x 1024 tiles (20 key bits)
constexpr float KEY_SHRINK = 1.0f - 1.0f / 65536.0f;
constexpr float KEY_GROW = 1.0f + 1.0f / 65536.0f;

struct Cam {
	float r[12];            // row-major [R | t] of the world-to-camera matrix
	float fx, fy, cx, cy;
	float z_near;
	int W, H, tiles_x, tiles_y;
	int cull;
};

__device__ __forceinline__ float3 cross3(float3 u, float3 v)
{
	return make_float3(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
}
// u x v with each component formed in fp64 (the products of two floats are exact there) and rounded to fp32 once: the
// edge functions of thin faces seen far off-axis keep their direction, and edge3(v, u) is the exact negative of edge3(u, v)
__device__ __forceinline__ float3 edge3(float3 u, float3 v)
{
	const double ux = u.x, uy = u.y, uz = u.z, vx = v.x, vy = v.y, vz = v.z;
	return make_float3((float)(uy * vz - uz * vy), (float)(uz * vx - ux * vz), (float)(ux * vy - uy * vx));
}
__device__ __forceinline__ float3 sub3(float3 u, float3 v) { return make_float3(u.x - v.x, u.y - v.y, u.z - v.z); }
__device__ __forceinline__ bool finite3(float3 u) { return isfinite(u.x) && isfinite(u.y) && isfinite(u.z); }
__device__ __forceinline__ bool eq3(float3 u, float3 v) { return u.x == v.x && u.y == v.y && u.z == v.z; }

// ------------------------------------------------------------------------------------------------------ per vertex
__global__ void __launch_bounds__(256) mesh_xform(const float* __restrict__ verts, int V, Cam cam, float4* __restrict__ vc)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= V) return;
	const float x = verts[3 * (size_t)i], y = verts[3 * (size_t)i + 1], z = verts[3 * (size_t)i + 2];
	const float* r = cam.r;
	vc[i] = make_float4(((r[0] * x + r[1] * y) + r[2] * z) + r[3], ((r[4] * x + r[5] * y) + r[6] * z) + r[7],
	                    ((r[8] * x + r[9] * y) + r[10] * z) + r[11], 0.0f);
}

// ------------------------------------------------------------------------------------------------------ per face
// the clipped polygon's extent along one image axis, in pixel units: u = f * p / z + c over the vertices with z > 0;
// vertices on the plane z = 0 (z_near = 0 only) stand for directions to infinity
struct Extent {
	double lo = INFINITY, hi = -INFINITY;
};
__device__ __forceinline__ void extent_add(Extent& e, double p, double z, double f, double c, double tol)
{
	if (z > 0.0) {
		const double u = f * (p / z) + c;
		e.lo = fmin(e.lo, u);
		e.hi = fmax(e.hi, u);
	} else {   // a point at infinity in direction sign(f * p)
		const double s = f * p;
		if (!(s < tol)) e.hi = INFINITY;
		if (!(s > -tol)) e.lo = -INFINITY;
	}
}
// first pixel index whose centre (+0.5) is >= lo - 1 and last whose centre is <= hi + 1, clamped to [0, n - 1]
__device__ __forceinline__ void pixel_span(const Extent& e, int n, int& p0, int& p1)
{
	const double a = fmax(ceil(e.lo - 1.5), 0.0), b = fmin(floor(e.hi + 0.5), (double)(n - 1));
	if (!(a <= b)) { p0 = 1; p1 = 0; return; }
	p0 = (int)a;
	p1 = (int)b;
}

// rec[3f..3f+2] = {e_a.xyz, e_b.x}, {e_b.yz, e_c.xy}, {e_c.z, z_a, z_b, z_c}; rect[f] = tile rect (x0, y0, x1, y1), x0 > x1 = culled;
// prect[f] = the pixel rect (x0 | x1 << 16, y0 | y1 << 16), each bound below MAX_DIM; key[f] = the lower bound of the face's hit z;
// cnt[f] = tiles of the rect
__global__ void __launch_bounds__(256) face_setup(const float4* __restrict__ vc, int V, const int* __restrict__ faces, int F, Cam cam,
                                                  float4* __restrict__ rec, int4* __restrict__ rect, uint2* __restrict__ prect,
                                                  float* __restrict__ key,
                                                  long long* __restrict__ cnt, int* status)
{
	const int f = blockIdx.x * 256 + threadIdx.x;
	if (f >= F) return;
	const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
	rect[f] = make_int4(1, 0, 0, 0);
	cnt[f] = 0;
	if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) {
		atomicOr(status, 1);
		return;
	}
	const float4 A = vc[ia], B = vc[ib], C = vc[ic];
	const float3 a = make_float3(A.x, A.y, A.z), b = make_float3(B.x, B.y, B.z), c = make_float3(C.x, C.y, C.z);
	// never hit: a non-finite vertex; two coincident vertices (then S = 0 exactly on every ray)
	if (!finite3(a) || !finite3(b) || !finite3(c) || eq3(a, b) || eq3(b, c) || eq3(c, a)) return;
	if (cam.cull) {   // front-facing: ((b - a) x (c - a)) . a < 0
		const float3 n = cross3(sub3(b, a), sub3(c, a));
		if (!(((n.x * a.x + n.y * a.y) + n.z * a.z) < 0.0f)) return;
	}
	// every hit z lies within [zmin, zmax] up to a few ulps: sum of three non-negative weights times z_k, weights summing to 1
	const float zmin = fminf(fminf(a.z, b.z), c.z), zmax = fmaxf(fmaxf(a.z, b.z), c.z);
	if (!((zmax > 0.0f ? zmax * KEY_GROW : zmax) > cam.z_near)) return;
	// + 0.0f turns a -0 (a vertex at camera z = -0 with z_near = 0) into +0: the key's bits are sorted as an unsigned integer
	const float kz = fmaxf(zmin > 0.0f ? zmin * KEY_SHRINK : zmin * KEY_GROW, cam.z_near) + 0.0f;

	// clip against z = zc (fp64) and take the projected extent of the clipped polygon
	const double zc = (double)cam.z_near * (1.0 - 1.0 / 4096.0);
	const double P[3][3] = {{a.x, a.y, a.z}, {b.x, b.y, b.z}, {c.x, c.y, c.z}};
	Extent ex, ey;
	for (int k = 0; k < 3; k++) {
		const double* p = P[k];
		const double* q = P[(k + 1) % 3];
		if (p[2] > zc) {
			extent_add(ex, p[0], p[2], cam.fx, cam.cx, 0.0);
			extent_add(ey, p[1], p[2], cam.fy, cam.cy, 0.0);
		}
		if ((p[2] > zc) != (q[2] > zc)) {   // the edge crosses the plane
			const double t = (zc - p[2]) / (q[2] - p[2]);
			const double x = p[0] + t * (q[0] - p[0]), y = p[1] + t * (q[1] - p[1]);
			const double tx = 1e-9 * (fabs(p[0]) + fabs(q[0])) * fabs((double)cam.fx);
			const double ty = 1e-9 * (fabs(p[1]) + fabs(q[1])) * fabs((double)cam.fy);
			extent_add(ex, x, zc, cam.fx, cam.cx, tx);
			extent_add(ey, y, zc, cam.fy, cam.cy, ty);
		}
	}
	int px0, px1, py0, py1;
	pixel_span(ex, cam.W, px0, px1);
	pixel_span(ey, cam.H, py0, py1);
	if (px0 > px1 || py0 > py1) return;
	const int4 r = make_int4(px0 / TILE, py0 / TILE, px1 / TILE, py1 / TILE);
	rect[f] = r;
	prect[f] = make_uint2((unsigned)px0 | (unsigned)px1 << 16, (unsigned)py0 | (unsigned)py1 << 16);
	cnt[f] = (long long)(r.z - r.x + 1) * (r.w - r.y + 1);
	key[f] = kz;
	const float3 ea = edge3(b, c), eb = edge3(c, a), ec = edge3(a, b);
	rec[3 * (size_t)f] = make_float4(ea.x, ea.y, ea.z, eb.x);
	rec[3 * (size_t)f + 1] = make_float4(eb.y, eb.z, ec.x, ec.y);
	rec[3 * (size_t)f + 2] = make_float4(ec.z, a.z, b.z, c.z);
}

// ------------------------------------------------------------------------------------------------------ binning
__global__ void __launch_bounds__(256) bin_emit(const int4* __restrict__ rect, const float* __restrict__ key,
                                                const long long* __restrict__ off, int F, int tiles_x, uint64_t* __restrict__ keys,
                                                int* __restrict__ vals)
{
	const int f = blockIdx.x * 256 + threadIdx.x;
	if (f >= F) return;
	const int4 r = rect[f];
	if (r.x > r.z) return;
	const uint64_t kb = (uint64_t)__float_as_uint(key[f]);   // key >= z_near >= 0: the bits order like the values
	long long o = off[f];
	for (int ty = r.y; ty <= r.w; ty++)
		for (int tx = r.x; tx <= r.z; tx++, o++) {
			keys[o] = ((uint64_t)(ty * tiles_x + tx) << 32) | kb;
			vals[o] = f;
		}
}
__global__ void __launch_bounds__(256) tile_ranges(const uint64_t* __restrict__ keys, int n, int2* __restrict__ ranges)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int t = (int)(keys[i] >> 32);
	if (i == 0 || (int)(keys[i - 1] >> 32) != t) ranges[t].x = i;
	if (i == n - 1 || (int)(keys[i + 1] >> 32) != t) ranges[t].y = i + 1;
}

// ------------------------------------------------------------------------------------------------------ the walk
__global__ void __launch_bounds__(256) mesh_walk(const int2* __restrict__ ranges, const uint64_t* __restrict__ keys,
                                                 const int* __restrict__ vals, const float4* __restrict__ rec,
                                                 const uint2* __restrict__ prect, Cam cam,
                                                 int* __restrict__ pix_to_face, float* __restrict__ zbuf, float* __restrict__ bary)
{
	__shared__ float4 s_r0[256], s_r1[256], s_r2[256];
	__shared__ float s_key[256];
	__shared__ int s_id[256];
	__shared__ uint2 s_pr[256];
	const int tile = blockIdx.x;
	const int tx = tile % cam.tiles_x, ty = tile / cam.tiles_x;
	const int j = tx * TILE + (int)(threadIdx.x % TILE), i = ty * TILE + (int)(threadIdx.x / TILE);
	const bool inside = i < cam.H && j < cam.W;
	const unsigned uj = (unsigned)j, ui = (unsigned)i;
	const float dx = (((float)j + 0.5f) - cam.cx) / cam.fx, dy = (((float)i + 0.5f) - cam.cy) / cam.fy;
	float bz = INFINITY, la = -1.0f, lb = -1.0f, lc = -1.0f;
	int bf = 0x7fffffff;
	bool done = !inside;
	const int2 rg = ranges[tile];
	for (int base = rg.x; base < rg.y; base += 256) {
		if (!__syncthreads_or(!done)) break;
		const int n = min(256, rg.y - base);
		if ((int)threadIdx.x < n) {
			const int f = vals[base + threadIdx.x];
			s_key[threadIdx.x] = __uint_as_float((uint32_t)keys[base + threadIdx.x]);
			s_id[threadIdx.x] = f;
			s_r0[threadIdx.x] = rec[3 * (size_t)f];
			s_r1[threadIdx.x] = rec[3 * (size_t)f + 1];
			s_r2[threadIdx.x] = rec[3 * (size_t)f + 2];
			s_pr[threadIdx.x] = prect[f];
		}
		__syncthreads();
		for (int k = 0; k < n; k++) {
			done = done || bz < s_key[k];   // faces come in ascending key order: no later face can go below bz
			if (__ballot(!done) == 0) break;
			if (done) continue;
			const float4 r0 = s_r0[k], r1 = s_r1[k], r2 = s_r2[k];
			const float Ea = (r0.x * dx + r0.y * dy) + r0.z;
			const float Eb = (r0.w * dx + r1.x * dy) + r1.y;
			const float Ec = (r1.z * dx + r1.w * dy) + r2.x;
			const bool pos = Ea >= 0.0f && Eb >= 0.0f && Ec >= 0.0f, neg = Ea <= 0.0f && Eb <= 0.0f && Ec <= 0.0f;
			const float S = (Ea + Eb) + Ec;
			const uint2 pr = s_pr[k];   // the face's pixel rectangle: outside it the face hits nothing
			const bool in = uj >= (pr.x & 0xffffu) && uj <= (pr.x >> 16) && ui >= (pr.y & 0xffffu) && ui <= (pr.y >> 16);
			if (!(pos || neg) || S == 0.0f || !in) continue;
			const float pa = Ea / S, pb = Eb / S, pc = Ec / S;
			const float z = (pa * r2.y + pb * r2.z) + pc * r2.w;
			const int f = s_id[k];
			if (z > cam.z_near && z < INFINITY && (z < bz || (z == bz && f < bf))) {
				bz = z; bf = f; la = pa; lb = pb; lc = pc;
			}
		}
		__syncthreads();
	}
	if (!inside) return;
	const size_t p = (size_t)i * cam.W + j;
	const bool hit = bf != 0x7fffffff;
	pix_to_face[p] = hit ? bf : -1;
	zbuf[p] = hit ? bz : -1.0f;
	bary[3 * p] = la;
	bary[3 * p + 1] = lb;
	bary[3 * p + 2] = lc;
}

// ------------------------------------------------------------------------------------------------------ helpers
// out[p, c] = (l_a A[fa, c] + l_b A[fb, c]) + l_c A[fc, c], 0 on background
__global__ void __launch_bounds__(256) mesh_interp(const int* __restrict__ faces, int F, const int* __restrict__ p2f,
                                                   const float* __restrict__ bary, int N, const float* __restrict__ attr, int V,
                                                   int C, float* __restrict__ out, int* status)
{
	const int p = blockIdx.x * 256 + threadIdx.x;
	if (p >= N) return;
	const int f = p2f[p];
	float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	if (f >= F) atomicOr(status, 1);
	if (f >= 0 && f < F) {
		const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
		if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) {
			atomicOr(status, 1);
		} else {
			const float wa = bary[3 * (size_t)p], wb = bary[3 * (size_t)p + 1], wc = bary[3 * (size_t)p + 2];
			for (int c = 0; c < C; c++)
				o[c] = (wa * attr[(size_t)ia * C + c] + wb * attr[(size_t)ib * C + c]) + wc * attr[(size_t)ic * C + c];
		}
	}
	for (int c = 0; c < C; c++) out[(size_t)p * C + c] = o[c];
}

__global__ void __launch_bounds__(256) corner_emit(const int* __restrict__ faces, long long n, int V, uint64_t* __restrict__ keys,
                                                   int* __restrict__ vals, int* status)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int v = faces[i];
	if (v < 0 || v >= V) atomicOr(status, 1);
	keys[i] = (uint64_t)(uint32_t)min(max(v, 0), V - 1);
	vals[i] = (int)i;
}
__global__ void __launch_bounds__(256) vertex_ranges(const uint64_t* __restrict__ keys, int n, int2* __restrict__ ranges)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int v = (int)keys[i];
	if (i == 0 || (int)keys[i - 1] != v) ranges[v].x = i;
	if (i == n - 1 || (int)keys[i + 1] != v) ranges[v].y = i + 1;
}
// Meshes.verts_normals_packed: corner k of face f adds (v_{k+1} - v_k) x (v_{k+2} - v_k), summed in ascending (f, k) order,
// then n / max(|n|, 1e-6)
__global__ void __launch_bounds__(256) vertex_normals(const float* __restrict__ verts, int V, const int* __restrict__ faces,
                                                      const int2* __restrict__ ranges, const int* __restrict__ corners,
                                                      float* __restrict__ normals)
{
	const int v = blockIdx.x * 256 + threadIdx.x;
	if (v >= V) return;
	const int2 r = ranges[v];
	float3 s = make_float3(0.0f, 0.0f, 0.0f);
	for (int e = r.x; e < r.y; e++) {
		const int q = corners[e];
		const int f = q / 3, k = q - 3 * f;
		const int i0 = faces[3 * (size_t)f + k], i1 = faces[3 * (size_t)f + (k + 1) % 3], i2 = faces[3 * (size_t)f + (k + 2) % 3];
		const float3 p0 = make_float3(verts[3 * (size_t)i0], verts[3 * (size_t)i0 + 1], verts[3 * (size_t)i0 + 2]);
		const float3 p1 = make_float3(verts[3 * (size_t)i1], verts[3 * (size_t)i1 + 1], verts[3 * (size_t)i1 + 2]);
		const float3 p2 = make_float3(verts[3 * (size_t)i2], verts[3 * (size_t)i2 + 1], verts[3 * (size_t)i2 + 2]);
		const float3 c = cross3(sub3(p1, p0), sub3(p2, p0));
		s = make_float3(s.x + c.x, s.y + c.y, s.z + c.z);
	}
	const float d = fmaxf(sqrtf((s.x * s.x + s.y * s.y) + s.z * s.z), 1e-6f);
	normals[3 * (size_t)v] = s.x / d;
	normals[3 * (size_t)v + 1] = s.y / d;
	normals[3 * (size_t)v + 2] = s.z / d;
}

__global__ void __launch_bounds__(256) visible_mark(const int* __restrict__ p2f, int N, int F, unsigned char* __restrict__ vis, int* status)
{
	const int p = blockIdx.x * 256 + threadIdx.x;
	if (p >= N) return;
	const int f = p2f[p];
	if (f >= F) atomicOr(status, 1);
	else if (f >= 0) vis[f] = 1;
}

}  // namespace

extern "C" {

int gsr_mesh_rasterize(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* verts, int num_verts, const int* faces,
                       int num_faces, const float intrinsics[9], const float extrinsics[16], int height, int width,
                       int cull_backfaces, float z_near, int* pix_to_face, float* zbuf, float* bary, void* stream)
{
	if (num_verts < 0 || num_faces < 0 || (num_verts > 0 && !verts) || (num_faces > 0 && !faces) || !intrinsics || !extrinsics)
		return GSR_ERR_ARG;
	if (height <= 0 || width <= 0 || height > MAX_DIM || width > MAX_DIM || !pix_to_face || !zbuf || !bary) return GSR_ERR_ARG;
	Cam cam;
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 4; c++) cam.r[4 * r + c] = extrinsics[4 * r + c];
	for (int k = 0; k < 12; k++)
		if (!isfinite(cam.r[k])) return GSR_ERR_ARG;
	cam.fx = intrinsics[0]; cam.fy = intrinsics[4]; cam.cx = intrinsics[2]; cam.cy = intrinsics[5];
	if (!isfinite(cam.fx) || !isfinite(cam.fy) || !isfinite(cam.cx) || !isfinite(cam.cy) || cam.fx == 0.0f || cam.fy == 0.0f)
		return GSR_ERR_ARG;
	if (!isfinite(z_near) || z_near < 0.0f) return GSR_ERR_ARG;
	cam.z_near = z_near;
	cam.W = width; cam.H = height;
	cam.tiles_x = (width + TILE - 1) / TILE; cam.tiles_y = (height + TILE - 1) / TILE;
	cam.cull = cull_backfaces ? 1 : 0;
	const int T = cam.tiles_x * cam.tiles_y;
	const int V = num_verts, F = num_faces;
	hipStream_t s = (hipStream_t)stream;

	// pass 1: per vertex / per face setup and the tile counts
	float4 *vc, *rec;
	int4* rect;
	uint2* prect;
	float* key;
	long long *cnt, *off, *part;
	int* status;
	int2* ranges;
	auto carve1 = [&](Arena& w1) {
		vc = w1.take<float4>(V);
		rec = w1.take<float4>(3 * (size_t)F);
		rect = w1.take<int4>(F);
		prect = w1.take<uint2>(F);
		key = w1.take<float>(F);
		cnt = w1.take<long long>(F);
		off = w1.take<long long>((size_t)F + 1);
		part = w1.take<long long>(scan_part_len(F));
		status = w1.take<int>(1);
		ranges = w1.take<int2>(T);
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve1)) return GSR_ERR_ALLOC;
	GSR_TRY(hipMemsetAsync(status, 0, sizeof(int), s));
	GSR_TRY(hipMemsetAsync(ranges, 0, sizeof(int2) * T, s));
	long long R = 0;
	int st = 0;
	if (F > 0) {
		if (V > 0) hipLaunchKernelGGL(mesh_xform, dim3(blocks(V)), dim3(256), 0, s, verts, V, cam, vc);
		hipLaunchKernelGGL(face_setup, dim3(blocks(F)), dim3(256), 0, s, vc, V, faces, F, cam, rec, rect, prect, key, cnt, status);
		const int rc = exclusive_scan<long long>(cnt, F, off, part, s);
		if (rc) return rc;
		GSR_TRY(hipMemcpyAsync(&R, off + F, sizeof(long long), hipMemcpyDeviceToHost, s));
		GSR_TRY(hipMemcpyAsync(&st, status, sizeof(int), hipMemcpyDeviceToHost, s));
		GSR_TRY(hipStreamSynchronize(s));
		if (st) return GSR_ERR_ARG;   // a face index outside [0, num_verts)
		if (R >= (1LL << 31) - 1) return GSR_ERR_ARG;
	}
	const int n = (int)R;

	// pass 2: (tile, key) sort of the binned faces and the walk
	uint64_t* k0 = nullptr;
	int* v0 = nullptr;
	if (n > 0) {
		SortBufs<uint64_t> sb;
		auto carve2 = [&](Arena& w2) {
			k0 = w2.take<uint64_t>(n);
			v0 = w2.take<int>(n);
			sb = sort_take<uint64_t>(w2, n);
		};
		if (!ws_carve(workspace_alloc, workspace_ctx, carve2)) return GSR_ERR_ALLOC;
		hipLaunchKernelGGL(bin_emit, dim3(blocks(F)), dim3(256), 0, s, rect, key, off, F, cam.tiles_x, k0, v0);
		const int rc = radix_sort(k0, v0, n, 32 + bits_for(T), sb, s);
		if (rc) return rc;
		hipLaunchKernelGGL(tile_ranges, dim3(blocks(n)), dim3(256), 0, s, k0, n, ranges);
	}
	hipLaunchKernelGGL(mesh_walk, dim3(T), dim3(256), 0, s, ranges, k0, v0, rec, prect, cam, pix_to_face, zbuf, bary);
	GSR_TRY(hipGetLastError());
	return n;
}

int gsr_mesh_interpolate(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const int* faces, int num_faces, const int* pix_to_face,
                         const float* bary, int num_pixels, const float* attr, int num_verts, int channels, float* out, void* stream)
{
	if (num_faces < 0 || num_pixels < 0 || num_verts < 0 || channels < 1 || channels > GSR_MESH_MAX_CHANNELS) return GSR_ERR_ARG;
	if (num_pixels == 0) return GSR_OK;
	if (!pix_to_face || !bary || !out || (num_faces > 0 && !faces) || (num_verts > 0 && !attr)) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	int* status;
	if (!ws_carve(workspace_alloc, workspace_ctx, [&](Arena& ws) { status = ws.take<int>(1); })) return GSR_ERR_ALLOC;
	GSR_TRY(hipMemsetAsync(status, 0, sizeof(int), s));
	hipLaunchKernelGGL(mesh_interp, dim3(blocks(num_pixels)), dim3(256), 0, s, faces, num_faces, pix_to_face, bary, num_pixels, attr,
	                   num_verts, channels, out, status);
	GSR_TRY(hipGetLastError());
	return read_status(status, s);
}

int gsr_mesh_vertex_normals(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* verts, int num_verts, const int* faces,
                            int num_faces, float* normals, void* stream)
{
	if (num_verts < 0 || num_faces < 0 || num_faces > 0x7fffffff / 3 || (num_verts > 0 && (!verts || !normals)) ||
	    (num_faces > 0 && !faces))
		return GSR_ERR_ARG;
	if (num_verts == 0) return num_faces > 0 ? GSR_ERR_ARG : GSR_OK;
	hipStream_t s = (hipStream_t)stream;
	const int n = 3 * num_faces;
	int *status, *v0 = nullptr;
	int2* ranges;
	uint64_t* k0 = nullptr;
	SortBufs<uint64_t> sb;
	auto carve = [&](Arena& ws) {
		status = ws.take<int>(1);
		ranges = ws.take<int2>(num_verts);
		if (n > 0) {
			k0 = ws.take<uint64_t>(n);
			v0 = ws.take<int>(n);
			sb = sort_take<uint64_t>(ws, n);
		}
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	GSR_TRY(hipMemsetAsync(status, 0, sizeof(int), s));
	GSR_TRY(hipMemsetAsync(ranges, 0, sizeof(int2) * num_verts, s));
	int* corners = nullptr;
	if (n > 0) {
		hipLaunchKernelGGL(corner_emit, dim3(blocks(n)), dim3(256), 0, s, faces, (long long)n, num_verts, k0, v0, status);
		int rc = read_status(status, s);   // an index outside [0, num_verts): nothing is written
		if (rc) return rc;
		rc = radix_sort(k0, v0, n, bits_for(num_verts), sb, s);
		if (rc) return rc;
		hipLaunchKernelGGL(vertex_ranges, dim3(blocks(n)), dim3(256), 0, s, k0, n, ranges);
		corners = v0;
	}
	hipLaunchKernelGGL(vertex_normals, dim3(blocks(num_verts)), dim3(256), 0, s, verts, num_verts, faces, ranges, corners, normals);
	GSR_TRY(hipGetLastError());
	return GSR_OK;
}

int gsr_mesh_visible_faces(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const int* pix_to_face, int num_pixels, int num_faces,
                           unsigned char* visible, void* stream)
{
	if (num_pixels < 0 || num_faces < 0 || (num_pixels > 0 && !pix_to_face) || (num_faces > 0 && !visible)) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	if (num_faces > 0) GSR_TRY(hipMemsetAsync(visible, 0, num_faces, s));
	if (num_pixels == 0) return GSR_OK;
	int* status;
	if (!ws_carve(workspace_alloc, workspace_ctx, [&](Arena& ws) { status = ws.take<int>(1); })) return GSR_ERR_ALLOC;
	GSR_TRY(hipMemsetAsync(status, 0, sizeof(int), s));
	hipLaunchKernelGGL(visible_mark, dim3(blocks(num_pixels)), dim3(256), 0, s, pix_to_face, num_pixels, num_faces, visible, status);
	GSR_TRY(hipGetLastError());
	return read_status(status, s);
}

}  // extern "C"
