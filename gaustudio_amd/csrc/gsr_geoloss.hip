// gsr_geoloss.hip -- the two geometric regularisers of 2D Gaussian surfel training on the surfel operator's allmap [7,H,W]:
// normal consistency (rendered normal against the normal of the rendered depth) and depth distortion, forward and backward
// (its definition to the bit: tests/geoloss_model.py; design: DESIGN.md s23).
//
//   d   = (1 - rho) nan_to_num(a0 / a1) + rho nan_to_num(a5)                     the blended depth
//   p   = d ((x - cx) / fx, (y - cy) / fy, 1)                                    camera-space point of pixel (x, y)
//   c   = (p(x, y+1) - p(x, y-1)) x (p(x+1, y) - p(x-1, y)),  n = c / max(|c|, 1e-12)   interior pixels; n = 0 on the border
//   e   = 1 - <(a2, a3, a4), n a1>                                               a1 is a constant in this factor
//   out = lambda_n mean(e) + lambda_d mean(a6)
//
// One workgroup of 256 lanes owns a 16 x 64 tile, as in gsr_loss.hip.  The forward builds d of the tile plus a 1-pixel halo
// in LDS; a lane then takes one column and 4 adjacent rows.  The backward is a gather: the depth of pixel q enters the stencils
// of its four neighbours, so the workgroup builds d with a 2-pixel halo, evaluates the 18 x 66 stencil CENTRES of the tile plus
// a 1-pixel halo -- dL/da and dL/db of c = a x b, six planes in LDS -- and pixel q adds the four it takes part in, against its
// own ray.  Nothing is saved by the forward.  The rays (x - cx) / fx and (y - cy) / fy of a tile's columns and rows are two small
// LDS tables, one correctly rounded divide each.
// No expression is fused: every product and sum below rounds once, in the order written (the library is built with
// -ffp-contract=off).  The sums of e and a6 are float64, in the fixed tree of gsr_loss.hip.  No atomics.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "../../include/gsrast.h"
#include "gsr_internal.h"
#include "gsr_ws.h"

namespace {

constexpr int TH = 16, TW = 64;           // the tile (surfel_losses.TILE_H / TILE_W)
constexpr float EPS = 1e-12f;             // F.normalize's eps

struct Cam { float fx, fy, cx, cy, rho, wexp; };   // wexp = 1 - rho

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float finite_or_zero(float v) { return finite_f(v) ? v : 0.f; }

// d of a tile plus HALO pixels on every side, zeros outside the image; the ray tables of its columns and rows.  request()
// issues every global load, store() writes LDS: the caller puts its own loads between the two, so that a workgroup waits for
// memory once.  An element outside the image reads the plane's first value and drops it.
template <int HALO> struct DepthTile {
	static constexpr int SH = TH + 2 * HALO, SW = TW + 2 * HALO, N = SH * SW, ITER = (N + 255) / 256;
	float v0[ITER], v1[ITER], v5[ITER];

	__device__ __forceinline__ void request(const float* __restrict__ allmap, size_t hw, int ox, int oy, int W, int H)
	{
#pragma unroll
		for (int k = 0; k < ITER; k++) {
			const int t = threadIdx.x + 256 * k, ly = t / SW, lx = t - ly * SW, gx = ox + lx, gy = oy + ly;
			const bool in = t < N && gx >= 0 && gx < W && gy >= 0 && gy < H;
			const size_t p = in ? (size_t)gy * W + gx : 0;
			v0[k] = allmap[p]; v1[k] = allmap[hw + p]; v5[k] = allmap[5 * hw + p];
		}
	}

	__device__ __forceinline__ void store(float* __restrict__ sd, float* __restrict__ srx, float* __restrict__ sry, int ox, int oy,
	                                      int W, int H, const Cam& cam)
	{
#pragma unroll
		for (int k = 0; k < ITER; k++) {
			const int t = threadIdx.x + 256 * k, ly = t / SW, lx = t - ly * SW, gx = ox + lx, gy = oy + ly;
			const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
			const float de = finite_or_zero(v0[k] / v1[k]), dm = finite_or_zero(v5[k]);
			if (t < N) sd[t] = in ? cam.wexp * de + cam.rho * dm : 0.f;
		}
		const int t = threadIdx.x;
		if (t < SW) srx[t] = ((float)(ox + t) - cam.cx) / cam.fx;
		else if (t >= 128 && t < 128 + SH) sry[t - 128] = ((float)(oy + t - 128) - cam.cy) / cam.fy;
	}
};

struct Stencil { float ax, ay, az, bx, by, bz, nx, ny, nz, den; bool through; };

// the stencil centred on LDS element (lx, ly) of a depth tile of row stride SW: a = p(down) - p(up), b = p(right) - p(left),
// n = a x b / max(|a x b|, eps).  `through`: the norm is not clamped (F.normalize: the gradient passes through |c| when
// |c| >= eps, and n = c / eps is linear in c otherwise).  A NaN norm stays NaN.
template <int SW> __device__ __forceinline__ Stencil stencil(const float* __restrict__ sd, const float* __restrict__ srx,
                                                             const float* __restrict__ sry, int lx, int ly)
{
	const float* c = sd + ly * SW + lx;
	const float dU = c[-SW], dD = c[SW], dL = c[-1], dR = c[1];
	const float rx = srx[lx], rxl = srx[lx - 1], rxr = srx[lx + 1], ry = sry[ly], ryu = sry[ly - 1], ryd = sry[ly + 1];
	Stencil s;
	s.ax = dD * rx - dU * rx;   s.ay = dD * ryd - dU * ryu; s.az = dD - dU;
	s.bx = dR * rxr - dL * rxl; s.by = dR * ry - dL * ry;   s.bz = dR - dL;
	const float cx = s.ay * s.bz - s.az * s.by, cy = s.az * s.bx - s.ax * s.bz, cz = s.ax * s.by - s.ay * s.bx;
	const float nrm = sqrtf((cx * cx + cy * cy) + cz * cz);
	s.through = !(nrm < EPS);
	s.den = nrm < EPS ? EPS : nrm;
	s.nx = cx / s.den; s.ny = cy / s.den; s.nz = cz / s.den;
	return s;
}

__device__ __forceinline__ bool interior(int gx, int gy, int W, int H) { return gx >= 1 && gx <= W - 2 && gy >= 1 && gy <= H - 2; }

// the fixed tree of gsr_loss.hip: 256 leaves, lane t adds leaf t + s for s = 128, 64, ..., 1
__device__ __forceinline__ void tree_reduce(double* red_a, double* red_b, double a, double b)
{
	const int t = threadIdx.x;
	red_a[t] = a; red_b[t] = b;
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if (t < s) { red_a[t] += red_a[t + s]; red_b[t] += red_b[t + s]; }
		__syncthreads();
	}
}

// maps (may be null) [10,H,W]: d_exp, d_med, d, n a1 (3), the rendered normal (3), e; view (may be null): 16 floats, the
// operator's viewmatrix as stored -- both normals of the MAPS become v -> sum_i v_i view[4 j + i] (surfel_renderer.py:101)
__global__ __launch_bounds__(256) void geoloss_fwd_kernel(const float* __restrict__ allmap, int W, int H, int tiles_x, Cam cam,
                                                          const float* __restrict__ view, float* __restrict__ maps,
                                                          double* __restrict__ partials)
{
	using DT = DepthTile<1>;
	__shared__ float s_d[DT::N];
	__shared__ float s_rx[DT::SW], s_ry[DT::SH];
	__shared__ double s_red[512];
	const int ty = blockIdx.x / (unsigned)tiles_x, tx = blockIdx.x - ty * tiles_x;
	const size_t hw = (size_t)H * W;
	const int ox = tx * TW - 1, oy = ty * TH - 1;
	DT dt;
	dt.request(allmap, hw, ox, oy, W, H);
	// the lane's own pixels: column cx, rows 4 rg .. 4 rg + 3
	const int t = threadIdx.x, cx = t & 63, rg = t >> 6, gx = tx * TW + cx;
	float al[4], n0[4], n1[4], n2[4], ds[4];
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const int gy = ty * TH + 4 * rg + i;
		const size_t p = (gx < W && gy < H) ? (size_t)gy * W + gx : 0;
		al[i] = allmap[hw + p]; n0[i] = allmap[2 * hw + p]; n1[i] = allmap[3 * hw + p]; n2[i] = allmap[4 * hw + p];
		ds[i] = allmap[6 * hw + p];
	}
	float R[9];
	if (maps && view) {
#pragma unroll
		for (int j = 0; j < 3; j++) { R[3 * j] = view[4 * j]; R[3 * j + 1] = view[4 * j + 1]; R[3 * j + 2] = view[4 * j + 2]; }
	}
	dt.store(s_d, s_rx, s_ry, ox, oy, W, H, cam);
	__syncthreads();

	double sum_e = 0.0, sum_d = 0.0;
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const int ly = 4 * rg + i, gy = ty * TH + ly;
		const bool inside = gx < W && gy < H;
		const Stencil s = stencil<DT::SW>(s_d, s_rx, s_ry, cx + 1, ly + 1);
		const bool inner = interior(gx, gy, W, H);
		const float sx = inner ? s.nx * al[i] : 0.f, sy = inner ? s.ny * al[i] : 0.f, sz = inner ? s.nz * al[i] : 0.f;
		const float e = 1.f - ((n0[i] * sx + n1[i] * sy) + n2[i] * sz);
		sum_e += inside ? (double)e : 0.0;
		sum_d += inside ? (double)ds[i] : 0.0;
		if (!inside || !maps) continue;
		const size_t p = (size_t)gy * W + gx;
		// the centre's own depths again, from the planes: three loads on the forward-only path
		const float a0 = allmap[p], a5 = allmap[5 * hw + p];
		maps[p] = finite_or_zero(a0 / al[i]);
		maps[hw + p] = finite_or_zero(a5);
		maps[2 * hw + p] = s_d[(ly + 1) * DT::SW + cx + 1];
		float sn[3] = {sx, sy, sz}, rn[3] = {n0[i], n1[i], n2[i]};
		if (view) {
#pragma unroll
			for (int j = 0; j < 3; j++) {
				sn[j] = (sx * R[3 * j] + sy * R[3 * j + 1]) + sz * R[3 * j + 2];
				rn[j] = (n0[i] * R[3 * j] + n1[i] * R[3 * j + 1]) + n2[i] * R[3 * j + 2];
			}
		}
#pragma unroll
		for (int j = 0; j < 3; j++) { maps[(3 + j) * hw + p] = sn[j]; maps[(6 + j) * hw + p] = rn[j]; }
		maps[9 * hw + p] = e;
	}
	tree_reduce(s_red, s_red + 256, sum_e, sum_d);
	if (t == 0) { partials[2 * (size_t)blockIdx.x] = s_red[0]; partials[2 * (size_t)blockIdx.x + 1] = s_red[256]; }
}

__global__ __launch_bounds__(256) void geoloss_final_kernel(const double* __restrict__ partials, int num_partials, double n,
                                                            float lambda_normal, float lambda_dist, float* __restrict__ out3)
{
	__shared__ double red[512];
	double a = 0.0, b = 0.0;
	for (int i = threadIdx.x; i < num_partials; i += 256) { a += partials[2 * (size_t)i]; b += partials[2 * (size_t)i + 1]; }
	tree_reduce(red, red + 256, a, b);
	if (threadIdx.x == 0) {
		const double nl = (double)lambda_normal * (red[0] / n), dl = (double)lambda_dist * (red[256] / n);
		out3[0] = (float)(nl + dl); out3[1] = (float)nl; out3[2] = (float)dl;
	}
}

// wn = lambda_n / (H W), wd = lambda_d / (H W), rounded once from float64 on the host
__global__ __launch_bounds__(256) void geoloss_bwd_kernel(const float* __restrict__ allmap, int W, int H, int tiles_x, Cam cam,
                                                          float wn, float wd, const float* __restrict__ grad_loss,
                                                          float* __restrict__ grad)
{
	using DT = DepthTile<2>;
	constexpr int CH = TH + 2, CW = TW + 2, CN = CH * CW, CITER = (CN + 255) / 256;   // the stencil centres: tile + 1
	__shared__ float s_d[DT::N];
	__shared__ float s_rx[DT::SW], s_ry[DT::SH];
	__shared__ float s_g[6 * CN];             // dL/da (3 planes), dL/db (3 planes) of every centre
	const int ty = blockIdx.x / (unsigned)tiles_x, tx = blockIdx.x - ty * tiles_x;
	const size_t hw = (size_t)H * W;
	const int ox = tx * TW - 2, oy = ty * TH - 2;
	DT dt;
	dt.request(allmap, hw, ox, oy, W, H);
	// alpha and the rendered normal of every centre
	float ca[CITER], c0[CITER], c1[CITER], c2[CITER];
#pragma unroll
	for (int k = 0; k < CITER; k++) {
		const int t = threadIdx.x + 256 * k, ly = t / CW, lx = t - ly * CW, gx = ox + 1 + lx, gy = oy + 1 + ly;
		const bool in = t < CN && gx >= 0 && gx < W && gy >= 0 && gy < H;
		const size_t p = in ? (size_t)gy * W + gx : 0;
		ca[k] = allmap[hw + p]; c0[k] = allmap[2 * hw + p]; c1[k] = allmap[3 * hw + p]; c2[k] = allmap[4 * hw + p];
	}
	// the lane's own pixels: column cx, rows 4 rg .. 4 rg + 3
	const int t = threadIdx.x, cx = t & 63, rg = t >> 6, gx = tx * TW + cx;
	float a0[4], a1[4], a5[4];
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const int gy = ty * TH + 4 * rg + i;
		const size_t p = (gx < W && gy < H) ? (size_t)gy * W + gx : 0;
		a0[i] = allmap[p]; a1[i] = allmap[hw + p]; a5[i] = allmap[5 * hw + p];
	}
	const float gup = *grad_loss;             // the upstream gradient of the scalar loss stays on the device
	dt.store(s_d, s_rx, s_ry, ox, oy, W, H, cam);
	__syncthreads();

	const float wng = gup * wn;
#pragma unroll
	for (int k = 0; k < CITER; k++) {
		const int u = threadIdx.x + 256 * k, ly = u / CW, lx = u - ly * CW, px = ox + 1 + lx, py = oy + 1 + ly;
		if (u >= CN) continue;
		float ga[3] = {0.f, 0.f, 0.f}, gb[3] = {0.f, 0.f, 0.f}, sn[3] = {0.f, 0.f, 0.f};
		if (interior(px, py, W, H)) {
			const Stencil s = stencil<DT::SW>(s_d, s_rx, s_ry, lx + 1, ly + 1);
			sn[0] = s.nx * ca[k]; sn[1] = s.ny * ca[k]; sn[2] = s.nz * ca[k];
			// dL/dn = -(gup wn a1) N, through the normalisation to dL/dc, through the cross product to dL/da and dL/db
			const float w = wng * ca[k];
			const float g0 = -(w * c0[k]), g1 = -(w * c1[k]), g2 = -(w * c2[k]);
			const float pr = s.through ? (s.nx * g0 + s.ny * g1) + s.nz * g2 : 0.f;
			const float q0 = (g0 - s.nx * pr) / s.den, q1 = (g1 - s.ny * pr) / s.den, q2 = (g2 - s.nz * pr) / s.den;
			ga[0] = s.by * q2 - s.bz * q1; ga[1] = s.bz * q0 - s.bx * q2; ga[2] = s.bx * q1 - s.by * q0;
			gb[0] = q1 * s.az - q2 * s.ay; gb[1] = q2 * s.ax - q0 * s.az; gb[2] = q0 * s.ay - q1 * s.ax;
		}
#pragma unroll
		for (int j = 0; j < 3; j++) { s_g[j * CN + u] = ga[j]; s_g[(3 + j) * CN + u] = gb[j]; }
		// a centre of the tile proper is a pixel this workgroup owns: its rendered normal's gradient, -(gup wn) n a1
		if (lx >= 1 && lx <= TW && ly >= 1 && ly <= TH && px < W && py < H) {
			const size_t p = (size_t)py * W + px;
#pragma unroll
			for (int j = 0; j < 3; j++) grad[(2 + j) * hw + p] = -(wng * sn[j]);
		}
	}
	__syncthreads();

	const float rx = s_rx[cx + 2];
	const float g6 = gup * wd;
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const int ly = 4 * rg + i, gy = ty * TH + ly;
		if (gx >= W || gy >= H) continue;
		const int c = (ly + 1) * CW + cx + 1;   // this pixel as a centre; it is the lower point of the centre above, ...
		float v[3];
#pragma unroll
		for (int j = 0; j < 3; j++)
			v[j] = (s_g[j * CN + c - CW] - s_g[j * CN + c + CW]) + (s_g[(3 + j) * CN + c - 1] - s_g[(3 + j) * CN + c + 1]);
		const float gd = (v[0] * rx + v[1] * s_ry[ly + 2]) + v[2];
		const float ge = cam.wexp * gd, q = a0[i] / a1[i];
		const bool fin = finite_f(q);
		const size_t p = (size_t)gy * W + gx;
		grad[p] = fin ? ge / a1[i] : 0.f;
		grad[hw + p] = fin ? -(ge * q) / a1[i] : 0.f;
		grad[5 * hw + p] = finite_f(a5[i]) ? cam.rho * gd : 0.f;
		grad[6 * hw + p] = g6;
	}
}

bool finite_host(float v) { return v - v == 0.f; }

// H, W >= 1, 7 H W and the number of tiles within int32; rho in [0, 1], finite lambdas >= 0, finite intrinsics, fx fy != 0
int plan(int height, int width, float fx, float fy, float cx, float cy, float depth_ratio, float lambda_normal, float lambda_dist,
         int* tiles_x, int* blocks, Cam* cam)
{
	if (height < 1 || width < 1 || 7LL * height * width > INT_MAX) return GSR_ERR_ARG;
	if (!(depth_ratio >= 0.f && depth_ratio <= 1.f)) return GSR_ERR_ARG;
	if (!finite_host(lambda_normal) || !finite_host(lambda_dist) || lambda_normal < 0.f || lambda_dist < 0.f) return GSR_ERR_ARG;
	if (!finite_host(fx) || !finite_host(fy) || !finite_host(cx) || !finite_host(cy) || fx == 0.f || fy == 0.f) return GSR_ERR_ARG;
	*tiles_x = (width + TW - 1) / TW;
	*blocks = *tiles_x * ((height + TH - 1) / TH);   // <= H W
	*cam = Cam{fx, fy, cx, cy, depth_ratio, 1.f - depth_ratio};
	return GSR_OK;
}

}  // namespace

extern "C" {

int gsr_surfel_geoloss_fwd(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* allmap, int height, int width, float fx,
                           float fy, float cx, float cy, float depth_ratio, float lambda_normal, float lambda_dist,
                           const float* viewmatrix, float* maps, float* out3, void* stream)
{
	int tiles_x, blocks;
	Cam cam;
	const int rc = plan(height, width, fx, fy, cx, cy, depth_ratio, lambda_normal, lambda_dist, &tiles_x, &blocks, &cam);
	if (rc != GSR_OK) return rc;
	if (!allmap || !out3 || !workspace_alloc) return GSR_ERR_ARG;
	double* partials = nullptr;
	if (!ws_carve(workspace_alloc, workspace_ctx, [&](Arena& ws) { partials = ws.take<double>(2 * (size_t)blocks); }))
		return GSR_ERR_ALLOC;
	hipStream_t s = (hipStream_t)stream;
	hipLaunchKernelGGL(geoloss_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, allmap, width, height, tiles_x, cam, viewmatrix,
	                   maps, partials);
	hipLaunchKernelGGL(geoloss_final_kernel, dim3(1), dim3(256), 0, s, partials, blocks, (double)height * (double)width,
	                   lambda_normal, lambda_dist, out3);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_surfel_geoloss_bwd(const float* allmap, int height, int width, float fx, float fy, float cx, float cy, float depth_ratio,
                           float lambda_normal, float lambda_dist, const float* grad_loss, float* grad_allmap, void* stream)
{
	int tiles_x, blocks;
	Cam cam;
	const int rc = plan(height, width, fx, fy, cx, cy, depth_ratio, lambda_normal, lambda_dist, &tiles_x, &blocks, &cam);
	if (rc != GSR_OK) return rc;
	if (!allmap || !grad_loss || !grad_allmap) return GSR_ERR_ARG;
	const double n = (double)height * (double)width;
	hipLaunchKernelGGL(geoloss_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, allmap, width, height, tiles_x,
	                   cam, (float)((double)lambda_normal / n), (float)((double)lambda_dist / n), grad_loss, grad_allmap);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
