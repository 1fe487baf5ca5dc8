// gsr_scaffold.hip -- Scaffold-GS inference in front of the operator: anchors + three small MLPs + camera -> Gaussians
// (gaustudio/renderers/scaffold_renderer.py get_gaussians_properties with its prefilter_voxel).  Contract: INTEGRATION.md
// s23 and tests/scaffold_model.py (the numpy model the GPU tests compare with bit for bit); design: DESIGN.md s20.
//
// Shape.  One lane per anchor, plain VALU.  The f32 MFMAs of gfx950 run at the vector rate and would fix neither the
// summation order nor save a cycle.  A lane holds x = [feat(32), view(3), dist(1)] and ONE hidden vector (32) in registers;
// the MLPs run one after the other.  The weights (28 KB) are wave-uniform: every pointer to them is a `const float*
// __restrict__` kernel argument indexed by compile-time or loop-uniform values only, so that they are read through the
// SCALAR cache (s_load_dwordx*) and enter the FMAs as SGPR operands; no weight is staged in LDS (its only use is a lane-
// private column for the hidden values of the rolled first layer, sc_layer1).  Every result is written by ordinary vector
// stores.
//
// Two passes, because the number of Gaussians depends on the data:
//   scaffold_count  all N anchors: visible filter (or the caller's mask), view direction, feature bank, opacity MLP ->
//                   kept bit mask (bit j: logit j > 0) and its popcount; invisible anchors count 0.  Then gsr_sort.h's
//                   exclusive scan (1024-element tiles) -> start[N + 1], and one 4-byte read of the total.
//   scaffold_emit   all N anchors, those with an empty mask leave at once: opacity MLP again (the same code on the same
//                   inputs: the same bits; the kept mask of the first pass, not the recomputed sign, decides what is
//                   written, so that a lane writes exactly start[a + 1] - start[a] rows), then the covariance MLP, then
//                   the colour MLP, each writing its own output array at start[a] + rank.
//
// Arithmetic.  -ffp-contract=off; every dot product is  acc = bias; acc = FMA(W[o][i], x[i], acc) for i ascending; the
// activations are built from gs_exp (argument <= 0, clamped at -80) and IEEE + - * / sqrt.  No atomics.
#include "gsr_common.h"
#include "gsr_sort.h"
#include "gsr_ws.h"

namespace {

constexpr int SC_FEAT = 32;          // anchor_feat = hidden width
constexpr int SC_IN = SC_FEAT + 4;   // [feat, view, dist]

// An empty asm the value passes through: the SLP vectoriser pairs the dot products of two output rows into v_pk_fma_f32
// (seeded by the adjacent stores and compares of their results), which needs the two rows' weights side by side in a
// register pair -- three instructions per packed fma instead of one v_fma_f32 with an SGPR operand per term.  Behind this
// the chains have no vectorisable user.  No instruction is emitted.
#define SC_OPAQUE(v) asm volatile("" : "+v"(v))

__device__ __forceinline__ float sc_clamp80(float t) { return t < -80.0f ? -80.0f : t; }   // a NaN stays a NaN

__device__ __forceinline__ float sc_sigmoid(float x)
{
	if (x >= 0.0f) {
		const float e = gs_exp(sc_clamp80(-x));
		return 1.0f / (1.0f + e);
	}
	const float e = gs_exp(sc_clamp80(x));
	return e / (1.0f + e);
}

// tanh of a kept logit (x > 0)
__device__ __forceinline__ float sc_tanh_pos(float x)
{
	const float e = gs_exp(sc_clamp80(-2.0f * x));
	return (1.0f - e) / (1.0f + e);
}

// The radius the operator's preprocess reports for a Gaussian at `p` with the given scale and rotation
// (gsr_kernels_fwd.hip preprocess_fwd_kernel: near plane, det == 0, the 0.3 low-pass, ceil(3 sqrt(lambda_max)), the
// zero-area tile rect), 0 for a culled one.  Opacity does not enter.
__device__ __forceinline__ int sc_radius(const float3 p, const float3 sc, const float4 q, const float* __restrict__ view,
                                         const float* __restrict__ proj, float mod, float tan_fovx, float tan_fovy, float focal_x,
                                         float focal_y, int W, int H, int gx, int gy)
{
	const float4 p_hom = xform4x4(p, proj);
	const float p_w = 1.0f / (p_hom.w + 0.0000001f);
	const float p_proj_x = p_hom.x * p_w, p_proj_y = p_hom.y * p_w;
	const float3 p_view = xform4x3(p, view);
	if (p_view.z <= 0.2f) return 0;
	float cov3D[6];
	cov3d_from_scale_rot(sc, mod, q, cov3D);
	Cov2D c;
	cov2d_common(p, focal_x, focal_y, tan_fovx, tan_fovy, cov3D, view, c);
	const float cov_x = c.cov.m[0][0] + 0.3f;
	const float cov_y = c.cov.m[0][1];
	const float cov_z = c.cov.m[1][1] + 0.3f;
	const float det = FMA(-cov_y, cov_y, cov_x * cov_z);
	if (det == 0.0f) return 0;
	const float mid = 0.5f * (cov_x + cov_z);
	const float disc = sqrtf(fmaxf(0.1f, FMA(mid, mid, -det)));
	const float lambda1 = mid + disc, lambda2 = mid - disc;
	const float my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
	const float pix_x = (float)((((double)p_proj_x + 1.0) * (double)W - 1.0) * 0.5);
	const float pix_y = (float)((((double)p_proj_y + 1.0) * (double)H - 1.0) * 0.5);
	const int r_ = (int)my_radius;
	const int rminx = min(gx, max(0, (int)((pix_x - r_) / GSR_BLOCK_X)));
	const int rminy = min(gy, max(0, (int)((pix_y - r_) / GSR_BLOCK_Y)));
	const int rmaxx = min(gx, max(0, (int)((pix_x + r_ + GSR_BLOCK_X - 1) / GSR_BLOCK_X)));
	const int rmaxy = min(gy, max(0, (int)((pix_y + r_ + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y)));
	if ((rmaxx - rminx) * (rmaxy - rminy) == 0) return 0;
	return r_;
}

// h = relu(W1 x + b1): W1 [32, NI] row-major; bias first, inputs ascending
// The loop over the 32 hidden units stays ROLLED, two rows per trip (72 weights in SGPRs): unrolled, the three first layers
// of scaffold_emit are 54 KB of straight-line code that every wave runs once.  A rolled loop cannot index registers, so each
// lane parks its hidden values in its own LDS column (hl[o * 256], conflict-free, no barrier: a lane reads what it wrote)
// and takes all 32 back into registers for the second layer.
template <int NI>
__device__ __forceinline__ void sc_layer1(const float* __restrict__ w1, const float* __restrict__ b1, const float* x, float* hl,
                                          float* h)
{
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
	for (int o = 0; o < SC_FEAT; o += 2) {
		float a0 = b1[o], a1 = b1[o + 1];
#pragma unroll
		for (int i = 0; i < NI; i++) {
			a0 = FMA(w1[o * NI + i], x[i], a0);
			a1 = FMA(w1[(o + 1) * NI + i], x[i], a1);
		}
		SC_OPAQUE(a0);
		SC_OPAQUE(a1);
		hl[o * 256] = a0 < 0.0f ? 0.0f : a0;   // relu that keeps a NaN, as torch.relu does
		hl[(o + 1) * 256] = a1 < 0.0f ? 0.0f : a1;
	}
#pragma unroll
	for (int o = 0; o < SC_FEAT; o++) h[o] = hl[o * 256];
}

// one output of the second layer: row `o` of W2 [out, 32]
__device__ __forceinline__ float sc_out(const float* __restrict__ w2, const float* __restrict__ b2, int o, const float* h)
{
	float acc = b2[o];
#pragma unroll
	for (int i = 0; i < SC_FEAT; i++) acc = FMA(w2[o * SC_FEAT + i], h[i], acc);
	SC_OPAQUE(acc);
	return acc;
}

// x = [feat' (32), view (3), dist (1)] of anchor a
template <bool BANK>
__device__ __forceinline__ void sc_input(const float* __restrict__ anchor, const float* __restrict__ feat,
                                         const float* __restrict__ campos, const float* __restrict__ kw1,
                                         const float* __restrict__ kb1, const float* __restrict__ kw2,
                                         const float* __restrict__ kb2, int a, float* hl, float* x)
{
	const float vx = anchor[3 * (size_t)a] - campos[0], vy = anchor[3 * (size_t)a + 1] - campos[1], vz = anchor[3 * (size_t)a + 2] - campos[2];
	const float d = sqrtf(FMA(vz, vz, FMA(vy, vy, vx * vx)));
	x[SC_FEAT] = vx / d;
	x[SC_FEAT + 1] = vy / d;
	x[SC_FEAT + 2] = vz / d;
	x[SC_FEAT + 3] = d;
	const float4* fp = reinterpret_cast<const float4*>(feat + (size_t)a * SC_FEAT);
	if (!BANK) {
#pragma unroll
		for (int i = 0; i < SC_FEAT / 4; i++) {
			const float4 v = fp[i];
			x[4 * i] = v.x; x[4 * i + 1] = v.y; x[4 * i + 2] = v.z; x[4 * i + 3] = v.w;
		}
		return;
	}
	float f[SC_FEAT];
#pragma unroll
	for (int i = 0; i < SC_FEAT / 4; i++) {
		const float4 v = fp[i];
		f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
	}
	float hb[SC_FEAT];
	sc_layer1<4>(kw1, kb1, x + SC_FEAT, hl, hb);
	const float o0 = sc_out(kw2, kb2, 0, hb), o1 = sc_out(kw2, kb2, 1, hb), o2 = sc_out(kw2, kb2, 2, hb);
	// softmax with the maximum taken out: every exponent <= 0
	float m = o0;
	m = o1 > m ? o1 : m;
	m = o2 > m ? o2 : m;
	const float e0 = gs_exp(sc_clamp80(o0 - m)), e1 = gs_exp(sc_clamp80(o1 - m)), e2 = gs_exp(sc_clamp80(o2 - m));
	const float s = (e0 + e1) + e2;
	const float w0 = e0 / s, w1 = e1 / s, w2 = e2 / s;
	// feat[:, ::4].repeat(4) w0 + feat[:, ::2].repeat(2) w1 + feat w2: repeat TILES, so channel c reads 4 (c mod 8) and 2 (c mod 16)
#pragma unroll
	for (int c = 0; c < SC_FEAT; c++) x[c] = (f[4 * (c % 8)] * w0 + f[2 * (c % 16)] * w1) + f[c] * w2;
}

template <bool BANK>
__global__ void __launch_bounds__(256) scaffold_count(
    int N, int K, const float* __restrict__ anchor, const float* __restrict__ feat, const float* __restrict__ scaling,
    const float* __restrict__ rot, const float* __restrict__ ow1, const float* __restrict__ ob1, const float* __restrict__ ow2,
    const float* __restrict__ ob2, const float* __restrict__ kw1, const float* __restrict__ kb1, const float* __restrict__ kw2,
    const float* __restrict__ kb2, const float* __restrict__ view, const float* __restrict__ proj, const float* __restrict__ campos,
    float mod, float tan_fovx, float tan_fovy, float focal_x, float focal_y, int W, int H, const unsigned char* __restrict__ visible_in,
    unsigned char* __restrict__ visible, int* __restrict__ radii, unsigned short* __restrict__ kept, int* __restrict__ count)
{
	__shared__ float s_h[SC_FEAT * 256];
	float* hl = s_h + threadIdx.x;
	const int a = blockIdx.x * 256 + threadIdx.x;
	if (a >= N) return;
	bool vis;
	int r = 0;
	if (visible_in != nullptr) {
		vis = visible_in[a] != 0;
	} else {
		const float3 p = {anchor[3 * (size_t)a], anchor[3 * (size_t)a + 1], anchor[3 * (size_t)a + 2]};
		const float3 sc = {scaling[6 * (size_t)a], scaling[6 * (size_t)a + 1], scaling[6 * (size_t)a + 2]};
		const float4 q = *reinterpret_cast<const float4*>(rot + 4 * (size_t)a);
		r = sc_radius(p, sc, q, view, proj, mod, tan_fovx, tan_fovy, focal_x, focal_y, W, H, (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X,
		              (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y);
		vis = r > 0;
	}
	uint32_t bits = 0;
	if (vis) {
		float x[SC_IN], h[SC_FEAT];
		sc_input<BANK>(anchor, feat, campos, kw1, kb1, kw2, kb2, a, hl, x);
		sc_layer1<SC_IN>(ow1, ob1, x, hl, h);
		for (int j = 0; j < K; j++)
			if (sc_out(ow2, ob2, j, h) > 0.0f) bits |= 1u << j;   // on the logit: tanh(o) > 0 without a transcendental; NaN drops
	}
	visible[a] = vis ? 1 : 0;
	if (radii != nullptr) radii[a] = r;
	kept[a] = (unsigned short)bits;
	count[a] = __popc(bits);
}

template <bool BANK>
__global__ void __launch_bounds__(256) scaffold_emit(
    int N, int K, int M, const float* __restrict__ anchor, const float* __restrict__ feat, const float* __restrict__ offset,
    const float* __restrict__ scaling, const float* __restrict__ ow1, const float* __restrict__ ob1, const float* __restrict__ ow2,
    const float* __restrict__ ob2, const float* __restrict__ cw1, const float* __restrict__ cb1, const float* __restrict__ cw2,
    const float* __restrict__ cb2, const float* __restrict__ rw1, const float* __restrict__ rb1, const float* __restrict__ rw2,
    const float* __restrict__ rb2, const float* __restrict__ kw1, const float* __restrict__ kb1, const float* __restrict__ kw2,
    const float* __restrict__ kb2, const float* __restrict__ campos, const unsigned short* __restrict__ kept,
    const int* __restrict__ start, float* __restrict__ xyz, float* __restrict__ colors, float* __restrict__ opacity,
    float* __restrict__ scales, float* __restrict__ rotations, int* __restrict__ anchor_index, int* __restrict__ offset_index)
{
	__shared__ float s_h[SC_FEAT * 256];
	float* hl = s_h + threadIdx.x;
	const int a = blockIdx.x * 256 + threadIdx.x;
	if (a >= N) return;
	const uint32_t bits = kept[a];
	if (bits == 0) return;
	const int s0 = start[a];
	// the rows of this lane: [s0, s0 + popc(bits)); a scan that disagrees with the masks writes nothing out of bounds
	if (s0 < 0 || (long long)s0 + __popc(bits) > (long long)M) return;
	float x[SC_IN], h[SC_FEAT];
	sc_input<BANK>(anchor, feat, campos, kw1, kb1, kw2, kb2, a, hl, x);
	float sc6[6];
#pragma unroll
	for (int i = 0; i < 6; i++) sc6[i] = scaling[6 * (size_t)a + i];
	const float ax = anchor[3 * (size_t)a], ay = anchor[3 * (size_t)a + 1], az = anchor[3 * (size_t)a + 2];

	// positions and indices
	int row = s0;
	for (int j = 0; j < K; j++) {
		if (!((bits >> j) & 1u)) continue;
		const float* op = offset + ((size_t)a * K + j) * 3;
		xyz[3 * (size_t)row] = ax + op[0] * sc6[0];
		xyz[3 * (size_t)row + 1] = ay + op[1] * sc6[1];
		xyz[3 * (size_t)row + 2] = az + op[2] * sc6[2];
		anchor_index[row] = a;
		offset_index[row] = j;
		row++;
	}
	// opacity = tanh(logit)
	sc_layer1<SC_IN>(ow1, ob1, x, hl, h);
	row = s0;
	for (int j = 0; j < K; j++) {
		if (!((bits >> j) & 1u)) continue;
		opacity[row] = sc_tanh_pos(sc_out(ow2, ob2, j, h));
		row++;
	}
	// scales = scaling[3:6] sigmoid(o[0:3]); rotations = o[3:7] / max(|o[3:7]|, 1e-12)
	sc_layer1<SC_IN>(cw1, cb1, x, hl, h);
	row = s0;
	for (int j = 0; j < K; j++) {
		if (!((bits >> j) & 1u)) continue;
		float o[7];
#pragma unroll
		for (int c = 0; c < 7; c++) o[c] = sc_out(cw2, cb2, 7 * j + c, h);
#pragma unroll
		for (int c = 0; c < 3; c++) scales[3 * (size_t)row + c] = sc6[3 + c] * sc_sigmoid(o[c]);
		const float n = sqrtf(FMA(o[6], o[6], FMA(o[5], o[5], FMA(o[4], o[4], o[3] * o[3]))));
		const float dn = n < 1e-12f ? 1e-12f : n;   // a NaN norm stays
		*reinterpret_cast<float4*>(rotations + 4 * (size_t)row) = make_float4(o[3] / dn, o[4] / dn, o[5] / dn, o[6] / dn);
		row++;
	}
	// colours = sigmoid(o)
	sc_layer1<SC_IN>(rw1, rb1, x, hl, h);
	row = s0;
	for (int j = 0; j < K; j++) {
		if (!((bits >> j) & 1u)) continue;
#pragma unroll
		for (int c = 0; c < 3; c++) colors[3 * (size_t)row + c] = sc_sigmoid(sc_out(rw2, rb2, 3 * j + c, h));
		row++;
	}
}

bool sc_sizes_ok(int n, int k) { return n >= 0 && n <= (1 << 24) && k >= 1 && k <= 16 && (long long)n * k < (1LL << 31); }

}  // namespace

extern "C" {

int gsr_scaffold_count(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* anchor, const float* anchor_feat,
                       const float* scaling, const float* rot, const float* const weights[16], int num_anchors, int n_offsets,
                       const float* viewmatrix, const float* projmatrix, const float* campos, float tanfovx, float tanfovy,
                       int image_width, int image_height, float scale_modifier, const unsigned char* visible_in,
                       unsigned char* visible, int* radii, unsigned short* kept, int* start, int* total, void* stream)
{
	const int N = num_anchors, K = n_offsets;
	if (!sc_sizes_ok(N, K) || !weights || !start || !total || !campos) return GSR_ERR_ARG;
	if (!visible_in && (!viewmatrix || !projmatrix || !radii || image_width <= 0 || image_height <= 0 || image_width > 65535 ||
	                    image_height > 65535))
		return GSR_ERR_ARG;
	for (int i = 0; i < 4; i++)
		if (!weights[i]) return GSR_ERR_ARG;
	const bool bank = weights[12] != nullptr;
	if (bank && (!weights[13] || !weights[14] || !weights[15])) return GSR_ERR_ARG;
	if (N > 0 && (!anchor || !anchor_feat || !visible || !kept || (!visible_in && (!scaling || !rot)))) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	int *count, *part;
	auto carve = [&](Arena& ws) { count = ws.take<int>(N); part = ws.take<int>(scan_part_len(N)); };
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	const float focal_y = image_height / (2.0f * tanfovy), focal_x = image_width / (2.0f * tanfovx);   // as the operator forms them
	if (N > 0) {
		auto kern = bank ? scaffold_count<true> : scaffold_count<false>;
		hipLaunchKernelGGL(kern, dim3(blocks(N)), dim3(256), 0, s, N, K, anchor, anchor_feat, scaling, rot, weights[0], weights[1],
		                   weights[2], weights[3], weights[12], weights[13], weights[14], weights[15], viewmatrix, projmatrix, campos,
		                   scale_modifier, tanfovx, tanfovy, focal_x, focal_y, image_width, image_height, visible_in, visible,
		                   visible_in ? (int*)nullptr : radii, kept, count);
	}
	const int rc = exclusive_scan(count, N, start, part, s);
	if (rc) return rc;
	int tot = 0;
	GSR_TRY(hipMemcpyAsync(&tot, start + N, sizeof(int), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	if (tot < 0 || (long long)tot > (long long)N * K) return GSR_ERR_HIP;
	*total = tot;
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_scaffold_emit(const float* anchor, const float* anchor_feat, const float* offset, const float* scaling,
                      const float* const weights[16], int num_anchors, int n_offsets, const float* campos, const unsigned short* kept,
                      const int* start, int num_gaussians, float* xyz, float* colors, float* opacity, float* scales, float* rotations,
                      int* anchor_index, int* offset_index, void* stream)
{
	const int N = num_anchors, K = n_offsets, M = num_gaussians;
	if (!sc_sizes_ok(N, K) || !weights || !campos || M < 0 || (long long)M > (long long)N * K) return GSR_ERR_ARG;
	for (int i = 0; i < 12; i++)
		if (!weights[i]) return GSR_ERR_ARG;
	const bool bank = weights[12] != nullptr;
	if (bank && (!weights[13] || !weights[14] || !weights[15])) return GSR_ERR_ARG;
	if (M == 0) return GSR_OK;
	if (!anchor || !anchor_feat || !offset || !scaling || !kept || !start || !xyz || !colors || !opacity || !scales || !rotations ||
	    !anchor_index || !offset_index)
		return GSR_ERR_ARG;
	auto kern = bank ? scaffold_emit<true> : scaffold_emit<false>;
	hipLaunchKernelGGL(kern, dim3(blocks(N)), dim3(256), 0, (hipStream_t)stream, N, K, M, anchor, anchor_feat, offset, scaling,
	                   weights[0], weights[1], weights[2], weights[3], weights[4], weights[5], weights[6], weights[7], weights[8],
	                   weights[9], weights[10], weights[11], weights[12], weights[13], weights[14], weights[15], campos, kept, start,
	                   xyz, colors, opacity, scales, rotations, anchor_index, offset_index);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
