// gsr_loss.hip -- the photometric loss Gaussian splatting is trained with, (1 - lambda) L1 + lambda (1 - SSIM), forward and
// backward (its definition to the bit: tests/loss_model.py; design: DESIGN.md s21).
//
// SSIM is the published 3DGS one: an 11 x 11 Gaussian window (sigma 1.5) under zero padding, separable.  One workgroup of 256
// lanes owns a 16 x 64 tile of one plane:
//   1. the tile and its 5-pixel halo, 26 x 74 values per source, go into LDS (zeros outside the image);
//   2. horizontal pass: a lane takes one halo row and 8 adjacent outputs, reads its 18 inputs per source as five 16-byte LDS
//      reads, forms the quantities (x, y, x^2, y^2, xy in the forward; the three saved maps in the backward) in registers and
//      writes the row sums TRANSPOSED, column-major, so that
//   3. vertical pass: a lane takes one column and 4 adjacent rows and reads its 14 inputs per quantity as four 16-byte reads.
// An output costs 10 / 8 + 20 / 4 = 6.25 LDS reads in the forward instead of 2 x 11 + 5 x 11.  Both LDS images have an odd
// number of 16-byte slots per row (76 and 28 floats), which spreads the lanes of a 16-byte read over the slots.
// Every dot product is g[0] v[0] first, then one fma per tap in ascending tap order.  The sums of ssim_map and |x - y| are
// float64: four pixels per lane in row order, a fixed 256-leaf tree per workgroup, one pair of partials per workgroup, and a
// one-workgroup kernel that adds the partials (lane t takes t, t + 256, ... in ascending order, then the same tree).  No atomics.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "../../include/gsrast.h"
#include "gsr_internal.h"
#include "gsr_ws.h"

namespace {

constexpr int TH = 16, TW = 64;           // the tile (losses.TILE_H / TILE_W)
constexpr int RAD = 5, TAPS = 11;
constexpr int SH = TH + 2 * RAD;          // 26 halo rows
constexpr int SW = TW + 2 * RAD;          // 74 halo columns
constexpr int SSTR = 76;                  // floats per row of a source image in LDS: 19 slots of 16 bytes
constexpr int HSTR = 28;                  // floats per column of a transposed row-sum image: 7 slots (26 rows used)
constexpr int HGROUPS = TW / 8;           // 8 outputs per lane in the horizontal pass
constexpr int SRC_FLOATS = SH * SSTR, HQ_FLOATS = TW * HSTR;

// exp(-(i - 5)^2 / (2 1.5^2)) / sum, evaluated in float64 and rounded once (tests/test_loss_model.py checks the table)
struct Win { float g[TAPS]; };
constexpr Win WINDOW = {{0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,
                         0x1.b43c4p-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}};
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

struct Tile { int tx, ty; size_t plane; };

__device__ __forceinline__ Tile tile_of(int tiles_x, int tiles_y)
{
	const unsigned b = blockIdx.x, rest = b / (unsigned)tiles_x;
	Tile t;
	t.tx = (int)(b - rest * (unsigned)tiles_x);
	t.ty = (int)(rest % (unsigned)tiles_y);
	t.plane = rest / (unsigned)tiles_y;
	return t;
}

// rows oy .. oy + 25, columns ox .. ox + 73 of NS planes into dst[s * SRC_FLOATS ...], zeros outside the image.  Every global
// load of the tile is issued before the first LDS store (an element outside reads the plane's first value and drops it): one
// memory latency per workgroup, not one per element.
template <int NS> __device__ __forceinline__ void load_halos(float* __restrict__ dst, const float* const (&src)[NS], int ox, int oy,
                                                             int W, int H)
{
	constexpr int ITER = (SH * SW + 255) / 256;
	float v[NS][ITER];
#pragma unroll
	for (int k = 0; k < ITER; k++) {
		const int t = threadIdx.x + 256 * k, ly = t / SW, lx = t - ly * SW, gx = ox + lx, gy = oy + ly;
		const bool in = t < SH * SW && gx >= 0 && gx < W && gy >= 0 && gy < H;
		const size_t p = in ? (size_t)gy * W + gx : 0;
#pragma unroll
		for (int s = 0; s < NS; s++) {
			const float f = src[s][p];
			v[s][k] = in ? f : 0.f;
		}
	}
#pragma unroll
	for (int k = 0; k < ITER; k++) {
		const int t = threadIdx.x + 256 * k, ly = t / SW, lx = t - ly * SW;
		if (t < SH * SW) {
#pragma unroll
			for (int s = 0; s < NS; s++) dst[s * SRC_FLOATS + ly * SSTR + lx] = v[s][k];
		}
	}
}

// NOUT adjacent outputs from NOUT + 10 inputs held in registers: the sliding window
template <int NOUT> __device__ __forceinline__ void conv_run(const float* v, const Win& w, float* out)
{
#pragma unroll
	for (int j = 0; j < NOUT; j++) {
		float acc = w.g[0] * v[j];
#pragma unroll
		for (int k = 1; k < TAPS; k++) acc = FMA(w.g[k], v[j + k], acc);
		out[j] = acc;
	}
}

template <int NF4> __device__ __forceinline__ void read_f4(const float* p, float* v)
{
#pragma unroll
	for (int k = 0; k < NF4; k++) {
		const float4 f = reinterpret_cast<const float4*>(p)[k];
		v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w;
	}
}

// row sums of one quantity, 8 outputs of halo row r starting at column 8 g, into the transposed image hq
__device__ __forceinline__ void hpass_store(const float* v, const Win& w, float* __restrict__ hq, int g, int r)
{
	float o[8];
	conv_run<8>(v, w, o);
#pragma unroll
	for (int j = 0; j < 8; j++) hq[(8 * g + j) * HSTR + r] = o[j];
}

// column sums of one quantity: rows 4 rg .. 4 rg + 3 of column cx
__device__ __forceinline__ void vpass(const float* __restrict__ hq, const Win& w, int cx, int rg, float* out)
{
	float v[16];
	read_f4<4>(hq + cx * HSTR + 4 * rg, v);
	conv_run<4>(v, w, out);
}

// the fixed tree: 256 leaves, lane t adds leaf t + s for s = 128, 64, ..., 1
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

__global__ __launch_bounds__(256) void photometric_fwd_kernel(const float* __restrict__ image, const float* __restrict__ target,
                                                              int W, int H, int tiles_x, int tiles_y, size_t total, Win w,
                                                              float* __restrict__ ssim_map, float* __restrict__ maps,
                                                              double* __restrict__ partials)
{
	__shared__ __align__(16) float s_src[2 * SRC_FLOATS];
	__shared__ __align__(16) float s_h[5 * HQ_FLOATS];
	const Tile tl = tile_of(tiles_x, tiles_y);
	const size_t base = tl.plane * (size_t)H * W;
	float* sx = s_src;
	float* sy = s_src + SRC_FLOATS;
	const float* const srcs[2] = {image + base, target + base};
	load_halos<2>(s_src, srcs, tl.tx * TW - RAD, tl.ty * TH - RAD, W, H);
	__syncthreads();

	const int t = threadIdx.x;
	if (t < SH * HGROUPS) {
		const int g = t / SH, r = t - g * SH;
		float x[20], y[20], v[18];   // 18 used: columns 8 g .. 8 g + 17 <= 73
		read_f4<5>(sx + r * SSTR + 8 * g, x);
		read_f4<5>(sy + r * SSTR + 8 * g, y);
		hpass_store(x, w, s_h, g, r);
		hpass_store(y, w, s_h + HQ_FLOATS, g, r);
#pragma unroll
		for (int k = 0; k < 18; k++) v[k] = x[k] * x[k];
		hpass_store(v, w, s_h + 2 * HQ_FLOATS, g, r);
#pragma unroll
		for (int k = 0; k < 18; k++) v[k] = y[k] * y[k];
		hpass_store(v, w, s_h + 3 * HQ_FLOATS, g, r);
#pragma unroll
		for (int k = 0; k < 18; k++) v[k] = x[k] * y[k];
		hpass_store(v, w, s_h + 4 * HQ_FLOATS, g, r);
	}
	__syncthreads();

	const int cx = t & 63, rg = t >> 6;
	float mu1[4], mu2[4], e11[4], e22[4], e12[4];
	vpass(s_h, w, cx, rg, mu1);
	vpass(s_h + HQ_FLOATS, w, cx, rg, mu2);
	vpass(s_h + 2 * HQ_FLOATS, w, cx, rg, e11);
	vpass(s_h + 3 * HQ_FLOATS, w, cx, rg, e22);
	vpass(s_h + 4 * HQ_FLOATS, w, cx, rg, e12);

	const int gx = tl.tx * TW + cx;
	double sum_s = 0.0, sum_l = 0.0;
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const int ly = 4 * rg + i, gy = tl.ty * TH + ly;
		const bool inside = gx < W && gy < H;
		const float xv = sx[(ly + RAD) * SSTR + cx + RAD], yv = sy[(ly + RAD) * SSTR + cx + RAD];
		const float mu1sq = mu1[i] * mu1[i], mu2sq = mu2[i] * mu2[i], mu12 = mu1[i] * mu2[i];
		const float s1 = e11[i] - mu1sq, s2 = e22[i] - mu2sq, s12 = e12[i] - mu12;
		const float a1 = 2.f * mu12 + C1, a2 = 2.f * s12 + C2;
		const float b1 = (mu1sq + mu2sq) + C1, b2 = (s1 + s2) + C2;
		const float den = b1 * b2;
		const float S = (a1 * a2) / den;
		sum_s += inside ? (double)S : 0.0;
		sum_l += inside ? (double)fabsf(xv - yv) : 0.0;
		if (!inside) continue;
		const size_t p = base + (size_t)gy * W + gx;
		if (ssim_map) ssim_map[p] = S;
		if (maps) {
			// the partial derivatives of ssim_map in (mu1, s1, s12), folded for the three convolutions of the backward
			const float dD = (2.f * a1) / den;                   // d/ds12
			const float dB = -(S / b2);                          // d/ds1
			const float dA = ((2.f * a2) / den) * (mu2[i] - mu1[i] * (a1 / b1));   // d/dmu1
			maps[p] = FMA(-mu2[i], dD, FMA(-(2.f * mu1[i]), dB, dA));
			maps[total + p] = dB;
			maps[2 * total + p] = dD;
		}
	}
	__syncthreads();   // every lane is done with s_h: it becomes the tree's scratch
	double* red = reinterpret_cast<double*>(s_h);
	tree_reduce(red, red + 256, sum_s, sum_l);
	if (t == 0) { partials[2 * (size_t)blockIdx.x] = red[0]; partials[2 * (size_t)blockIdx.x + 1] = red[256]; }
}

__global__ __launch_bounds__(256) void photometric_final_kernel(const double* __restrict__ partials, int num_partials, double n,
                                                                float lambda_dssim, float* __restrict__ out3)
{
	__shared__ double red[512];
	double a = 0.0, b = 0.0;
	for (int i = threadIdx.x; i < num_partials; i += 256) { a += partials[2 * (size_t)i]; b += partials[2 * (size_t)i + 1]; }
	tree_reduce(red, red + 256, a, b);
	if (threadIdx.x == 0) {
		const double ssim = red[0] / n, l1 = red[256] / n, ld = (double)lambda_dssim;
		const double loss = (1.0 - ld) * l1 + ld * (1.0 - ssim);
		out3[0] = (float)loss; out3[1] = (float)l1; out3[2] = (float)ssim;
	}
}

__global__ __launch_bounds__(256) void photometric_bwd_kernel(const float* __restrict__ image, const float* __restrict__ target,
                                                              const float* __restrict__ maps, int W, int H, int tiles_x, int tiles_y,
                                                              size_t total, Win w, float w_l1, float w_ssim,
                                                              const float* __restrict__ grad_loss, float* __restrict__ grad_image)
{
	__shared__ __align__(16) float s_src[3 * SRC_FLOATS];
	__shared__ __align__(16) float s_h[3 * HQ_FLOATS];
	const Tile tl = tile_of(tiles_x, tiles_y);
	const size_t base = tl.plane * (size_t)H * W;
	const float* const srcs[3] = {maps + base, maps + total + base, maps + 2 * total + base};
	load_halos<3>(s_src, srcs, tl.tx * TW - RAD, tl.ty * TH - RAD, W, H);
	// the pixels' own x and y, used once at the end: requested now, the same way (a pixel outside reads the plane's first value)
	const int gx = tl.tx * TW + (threadIdx.x & 63);
	float xs[4], ys[4];
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const int gy = tl.ty * TH + 4 * (threadIdx.x >> 6) + i;
		const size_t p = base + ((gx < W && gy < H) ? (size_t)gy * W + gx : 0);
		xs[i] = image[p]; ys[i] = target[p];
	}
	__syncthreads();

	const int t = threadIdx.x;
	if (t < SH * HGROUPS) {
		const int g = t / SH, r = t - g * SH;
#pragma unroll
		for (int q = 0; q < 3; q++) {
			float v[20];
			read_f4<5>(s_src + q * SRC_FLOATS + r * SSTR + 8 * g, v);
			hpass_store(v, w, s_h + q * HQ_FLOATS, g, r);
		}
	}
	__syncthreads();

	const int cx = t & 63, rg = t >> 6;
	float c0[4], c1[4], c2[4];
	vpass(s_h, w, cx, rg, c0);
	vpass(s_h + HQ_FLOATS, w, cx, rg, c1);
	vpass(s_h + 2 * HQ_FLOATS, w, cx, rg, c2);
	const float gup = *grad_loss;   // the upstream gradient of the scalar loss stays on the device
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const int gy = tl.ty * TH + 4 * rg + i;
		if (gx >= W || gy >= H) continue;
		const size_t p = base + (size_t)gy * W + gx;
		const float xv = xs[i], yv = ys[i];
		const float dssim = FMA(yv, c2[i], FMA(2.f * xv, c1[i], c0[i]));
		const float d = xv - yv;
		const float sgn = (float)(0.f < d) - (float)(d < 0.f);   // torch.sign: 0 at 0
		grad_image[p] = gup * FMA(w_l1, sgn, -(w_ssim * dssim));
	}
}

// planes, H, W >= 1, planes H W and the number of tiles within int32
int plan(long long planes, int height, int width, int* tiles_x, int* tiles_y, long long* blocks)
{
	if (planes < 1 || height < 1 || width < 1 || planes > INT_MAX) return GSR_ERR_ARG;
	if (planes * (long long)height > INT_MAX || planes * (long long)height * width > INT_MAX) return GSR_ERR_ARG;
	*tiles_x = (width + TW - 1) / TW;
	*tiles_y = (height + TH - 1) / TH;
	*blocks = planes * *tiles_x * *tiles_y;   // <= planes H W
	return GSR_OK;
}

}  // namespace

extern "C" {

int gsr_photometric_fwd(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* image, const float* target,
                        long long planes, int height, int width, float lambda_dssim, float* ssim_map, float* maps, float* out3,
                        void* stream)
{
	int tiles_x, tiles_y;
	long long blocks;
	const int rc = plan(planes, height, width, &tiles_x, &tiles_y, &blocks);
	if (rc != GSR_OK) return rc;
	if (!image || !target || !out3 || !workspace_alloc || !(lambda_dssim >= 0.f && lambda_dssim <= 1.f)) return GSR_ERR_ARG;
	double* partials = nullptr;
	if (!ws_carve(workspace_alloc, workspace_ctx, [&](Arena& ws) { partials = ws.take<double>(2 * (size_t)blocks); }))
		return GSR_ERR_ALLOC;
	hipStream_t s = (hipStream_t)stream;
	const size_t total = (size_t)planes * height * width;
	hipLaunchKernelGGL(photometric_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, image, target, width, height, tiles_x,
	                   tiles_y, total, WINDOW, ssim_map, maps, partials);
	hipLaunchKernelGGL(photometric_final_kernel, dim3(1), dim3(256), 0, s, partials, (int)blocks, (double)total, lambda_dssim, out3);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_photometric_bwd(const float* image, const float* target, const float* maps, long long planes, int height, int width,
                        float lambda_dssim, const float* grad_loss, float* grad_image, void* stream)
{
	int tiles_x, tiles_y;
	long long blocks;
	const int rc = plan(planes, height, width, &tiles_x, &tiles_y, &blocks);
	if (rc != GSR_OK) return rc;
	if (!image || !target || !maps || !grad_loss || !grad_image || !(lambda_dssim >= 0.f && lambda_dssim <= 1.f)) return GSR_ERR_ARG;
	const size_t total = (size_t)planes * height * width;
	const double ld = (double)lambda_dssim, n = (double)total;
	hipLaunchKernelGGL(photometric_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, image, target, maps, width,
	                   height, tiles_x, tiles_y, total, WINDOW, (float)((1.0 - ld) / n), (float)(ld / n), grad_loss, grad_image);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
