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
//
// The gradient of the two passes (gsr_scaffold_backward; INTEGRATION.md s23a, tests/scaffold_grad_model.py)
// is further down: it recomputes the forward with the functions of this file, so its values are the forward's bits.
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

// the feature bank: hb = relu(kw1 vd + kb1), w = softmax(kw2 hb + kb2) with the maximum taken out: every exponent <= 0
__device__ __forceinline__ void sc_bank_w(const float* __restrict__ kw1, const float* __restrict__ kb1, const float* __restrict__ kw2,
                                          const float* __restrict__ kb2, const float* vd, float* hl, float* hb, float* w)
{
	sc_layer1<4>(kw1, kb1, vd, hl, hb);
	const float o0 = sc_out(kw2, kb2, 0, hb), o1 = sc_out(kw2, kb2, 1, hb), o2 = sc_out(kw2, kb2, 2, hb);
	float m = o0;
	m = o1 > m ? o1 : m;
	m = o2 > m ? o2 : m;
	const float e0 = gs_exp(sc_clamp80(o0 - m)), e1 = gs_exp(sc_clamp80(o1 - m)), e2 = gs_exp(sc_clamp80(o2 - m));
	const float s = (e0 + e1) + e2;
	w[0] = e0 / s;
	w[1] = e1 / s;
	w[2] = e2 / s;
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
	float hb[SC_FEAT], w[3];
	sc_bank_w(kw1, kb1, kw2, kb2, x + SC_FEAT, hl, hb, w);
	const float w0 = w[0], w1 = w[1], w2 = w[2];
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

// ------------------------------------------------------------------------------------------------------------ backward
// The gradient of decode (tests/scaffold_grad_model.py; design: DESIGN.md s20a).  Three kernels:
//   scaffold_bwd_anchor  one lane per anchor, as scaffold_emit: recomputes the forward with the forward's own functions,
//                        turns the cotangents of its rows into d anchor / anchor_feat / offset / scaling (plain stores into
//                        pre-zeroed outputs) and STAGES, per anchor, the factors of the weight gradients: the "left" rows
//                        (dout of every output, dpre of every hidden unit) and the "right" vectors (h of each MLP, x).
//   scaffold_bwd_wsum    dW = sum over anchors of left (x) right: a register-blocked VALU GEMM with the anchor index as
//                        K.  Blocks of 256 anchors are dealt to SB_CHAINS chains, block b to chain b mod SB_CHAINS; a chain
//                        walks its anchors in ascending order, one fma per anchor and element.  A lane owns 4 rows x 8 columns.
//   scaffold_bwd_final   adds the chains' partials in ascending chain order in float64 and writes the weight tensors.
// A launch covers one CHUNK of SB_CHAINS blocks (65536 anchors: the staging buffer is bounded by that), one block per chain;
// the chains' accumulators pass from chunk to chunk through the partials buffer, which changes no bit.
//
// Row space ("left" rows; each segment padded to a multiple of 4, rows of one lane share their right vector):
//   [dout opacity: k][dpre opacity: 32][dout cov: 7k][dpre cov: 32][dout colour: 3k][dpre colour: 32][dout bank: 3][dpre bank: 32]
// Right vectors (LDS slots of SB_SLOT floats, the value 1 behind the last entry gives the bias gradient):
//   0 h opacity, 1 h cov, 2 h colour, 3 x (36), 4 h bank, 5 (view, dist).
constexpr int SB_CHAINS = 256;                       // constant: depends on no device property
constexpr int SB_TILE = 32;                          // anchors per LDS tile
constexpr int SB_SLOT = 40;                          // columns per row: 5 column groups of 8
constexpr int SB_LROWS = 208;                        // left rows one workgroup can own: 52 row groups of 4
constexpr int SB_STRIDE = SB_LROWS + 6 * SB_SLOT + 4;   // 452 floats per anchor: = 4 mod 64, 16-byte aligned
constexpr int SB_RIGHT = 3 * SC_FEAT + SC_IN + SC_FEAT;   // staged right values per anchor: 164 (132 without the bank)

struct ScRows {
	int pk, p7, p3, lpad;
	int o_op, o_dop, o_cov, o_dcov, o_col, o_dcol, o_bank, o_dbank;
};

__host__ __device__ inline ScRows sc_rows(int K, bool bank)
{
	ScRows r;
	r.pk = (K + 3) & ~3;
	r.p7 = (7 * K + 3) & ~3;
	r.p3 = (3 * K + 3) & ~3;
	r.o_op = 0;
	r.o_dop = r.pk;
	r.o_cov = r.o_dop + SC_FEAT;
	r.o_dcov = r.o_cov + r.p7;
	r.o_col = r.o_dcov + SC_FEAT;
	r.o_dcol = r.o_col + r.p3;
	r.o_bank = r.o_dcol + SC_FEAT;
	r.o_dbank = r.o_bank + 4;
	r.lpad = bank ? r.o_dbank + SC_FEAT : r.o_bank;
	return r;
}

// dh += W2[o,:] dout
__device__ __forceinline__ void sc_dh(const float* __restrict__ w2, int o, float dout, float* dh)
{
#pragma unroll
	for (int i = 0; i < SC_FEAT; i++) dh[i] = FMA(w2[o * SC_FEAT + i], dout, dh[i]);
}

// dpre = dh where h > 0 (torch's relu rule: 0 at 0, 0 for a NaN); stages h and dpre; dx[c] = fma(W1[i][c], dpre[i], dx[c]) for
// i ascending, rolled like sc_layer1 (dpre parked in the lane's LDS column)
template <int NI>
__device__ __forceinline__ void sc_hidden_bwd(const float* __restrict__ w1, const float* h, const float* dh, float* hl, float* dx,
                                              float* st_dpre, float* st_h, size_t cap)
{
#pragma unroll
	for (int i = 0; i < SC_FEAT; i++) {
		const float dp = h[i] > 0.0f ? dh[i] : 0.0f;
		st_h[i * cap] = h[i];
		st_dpre[i * cap] = dp;
		hl[i * 256] = dp;
	}
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
	for (int i = 0; i < SC_FEAT; i++) {
		const float d = hl[i * 256];
#pragma unroll
		for (int c = 0; c < NI; c++) dx[c] = FMA(w1[i * NI + c], d, dx[c]);
	}
}

template <bool BANK>
__global__ void __launch_bounds__(256) scaffold_bwd_anchor(
    int N, int K, int M, int block0, size_t cap, const float* __restrict__ anchor, const float* __restrict__ feat,
    const float* __restrict__ offset, const float* __restrict__ scaling, const float* __restrict__ ow1, const float* __restrict__ ob1,
    const float* __restrict__ ow2, const float* __restrict__ ob2, const float* __restrict__ cw1, const float* __restrict__ cb1,
    const float* __restrict__ cw2, const float* __restrict__ cb2, const float* __restrict__ rw1, const float* __restrict__ rb1,
    const float* __restrict__ rw2, const float* __restrict__ rb2, const float* __restrict__ kw1, const float* __restrict__ kb1,
    const float* __restrict__ kw2, const float* __restrict__ kb2, const float* __restrict__ campos,
    const unsigned short* __restrict__ kept, const int* __restrict__ start, const float* __restrict__ gxyz,
    const float* __restrict__ gcol, const float* __restrict__ gop, const float* __restrict__ gsc, const float* __restrict__ grot,
    float* __restrict__ stage, float* __restrict__ d_anchor, float* __restrict__ d_feat, float* __restrict__ d_offset,
    float* __restrict__ d_scaling)
{
	__shared__ float s_h[SC_FEAT * 256];
	float* hl = s_h + threadIdx.x;
	const int a = (block0 + blockIdx.x) * 256 + threadIdx.x;
	if (a >= N) return;
	const uint32_t bits = kept[a];
	if (bits == 0) return;   // the outputs are pre-zeroed; scaffold_bwd_wsum reads nothing of this anchor
	const int s0 = start[a];
	if (s0 < 0 || (long long)s0 + __popc(bits) > (long long)M) return;   // as scaffold_emit; scaffold_bwd_wsum applies the same test
	const ScRows R = sc_rows(K, BANK);
	float* st = stage + (size_t)blockIdx.x * 256 + threadIdx.x;   // value v of this anchor: st[v * cap]
	float* sr = st + (size_t)R.lpad * cap;                        // the right values
	float x[SC_IN], h[SC_FEAT], dh[SC_FEAT], dx[SC_IN];
	sc_input<BANK>(anchor, feat, campos, kw1, kb1, kw2, kb2, a, hl, x);
#pragma unroll
	for (int i = 0; i < SC_IN; i++) {
		dx[i] = 0.0f;
		sr[(size_t)(3 * SC_FEAT + i) * cap] = x[i];
	}
	float sc6[6], ds6[6];
#pragma unroll
	for (int i = 0; i < 6; i++) {
		sc6[i] = scaling[6 * (size_t)a + i];
		ds6[i] = 0.0f;
	}

	// xyz = A + O S[0:3]
	float ga0 = 0.0f, ga1 = 0.0f, ga2 = 0.0f;
	int row = s0;
	if (gxyz != nullptr) {
		for (int j = 0; j < K; j++) {
			if (!((bits >> j) & 1u)) continue;
			const float* op = offset + ((size_t)a * K + j) * 3;
			float* dop = d_offset + ((size_t)a * K + j) * 3;
			const float g0 = gxyz[3 * (size_t)row], g1 = gxyz[3 * (size_t)row + 1], g2 = gxyz[3 * (size_t)row + 2];
			ga0 = ga0 + g0;
			ga1 = ga1 + g1;
			ga2 = ga2 + g2;
			dop[0] = g0 * sc6[0];
			dop[1] = g1 * sc6[1];
			dop[2] = g2 * sc6[2];
			ds6[0] = FMA(g0, op[0], ds6[0]);
			ds6[1] = FMA(g1, op[1], ds6[1]);
			ds6[2] = FMA(g2, op[2], ds6[2]);
			row++;
		}
	}

	// opacity = tanh(l): dl = G (1 - opacity^2)
	sc_layer1<SC_IN>(ow1, ob1, x, hl, h);
#pragma unroll
	for (int i = 0; i < SC_FEAT; i++) dh[i] = 0.0f;
	row = s0;
	for (int j = 0; j < R.pk; j++) {
		float dl = 0.0f;
		if (j < K && ((bits >> j) & 1u)) {
			const float o = sc_tanh_pos(sc_out(ow2, ob2, j, h));
			const float g = gop != nullptr ? gop[row] : 0.0f;
			dl = g * (1.0f - o * o);
			sc_dh(ow2, j, dl, dh);
			row++;
		}
		st[(size_t)(R.o_op + j) * cap] = dl;
	}
	sc_hidden_bwd<SC_IN>(ow1, h, dh, hl, dx, st + (size_t)R.o_dop * cap, sr, cap);

	// scales = S[3+c] sigmoid(u_c); rotations = u / max(|u|, 1e-12)
	sc_layer1<SC_IN>(cw1, cb1, x, hl, h);
#pragma unroll
	for (int i = 0; i < SC_FEAT; i++) dh[i] = 0.0f;
	row = s0;
	for (int j = 0; j < K; j++) {
		float du[7];
#pragma unroll
		for (int c = 0; c < 7; c++) du[c] = 0.0f;
		if ((bits >> j) & 1u) {
			float o[7];
#pragma unroll
			for (int c = 0; c < 7; c++) o[c] = sc_out(cw2, cb2, 7 * j + c, h);
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const float sg = sc_sigmoid(o[c]);
				const float g = gsc != nullptr ? gsc[3 * (size_t)row + c] : 0.0f;
				du[c] = (g * sc6[3 + c]) * (sg * (1.0f - sg));
				ds6[3 + c] = FMA(g, sg, ds6[3 + c]);
			}
			float g4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
			if (grot != nullptr) {
				const float4 gv = *reinterpret_cast<const float4*>(grot + 4 * (size_t)row);
				g4[0] = gv.x; g4[1] = gv.y; g4[2] = gv.z; g4[3] = gv.w;
			}
			const float n = sqrtf(FMA(o[6], o[6], FMA(o[5], o[5], FMA(o[4], o[4], o[3] * o[3]))));
			if (n < 1e-12f) {   // torch's clamp_min rule: the norm is a constant below the clamp
#pragma unroll
				for (int c = 0; c < 4; c++) du[3 + c] = g4[c] / 1e-12f;
			} else {
				const float r0 = o[3] / n, r1 = o[4] / n, r2 = o[5] / n, r3 = o[6] / n;
				const float dot = FMA(r3, g4[3], FMA(r2, g4[2], FMA(r1, g4[1], r0 * g4[0])));
				du[3] = (g4[0] - r0 * dot) / n;
				du[4] = (g4[1] - r1 * dot) / n;
				du[5] = (g4[2] - r2 * dot) / n;
				du[6] = (g4[3] - r3 * dot) / n;
			}
#pragma unroll
			for (int c = 0; c < 7; c++) sc_dh(cw2, 7 * j + c, du[c], dh);
			row++;
		}
#pragma unroll
		for (int c = 0; c < 7; c++) st[(size_t)(R.o_cov + 7 * j + c) * cap] = du[c];
	}
	for (int o = 7 * K; o < R.p7; o++) st[(size_t)(R.o_cov + o) * cap] = 0.0f;
	sc_hidden_bwd<SC_IN>(cw1, h, dh, hl, dx, st + (size_t)R.o_dcov * cap, sr + (size_t)SC_FEAT * cap, cap);

	// colors = sigmoid(z): dz = G c (1 - c)
	sc_layer1<SC_IN>(rw1, rb1, x, hl, h);
#pragma unroll
	for (int i = 0; i < SC_FEAT; i++) dh[i] = 0.0f;
	row = s0;
	for (int j = 0; j < K; j++) {
		float dz[3] = {0.0f, 0.0f, 0.0f};
		if ((bits >> j) & 1u) {
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const float sg = sc_sigmoid(sc_out(rw2, rb2, 3 * j + c, h));
				const float g = gcol != nullptr ? gcol[3 * (size_t)row + c] : 0.0f;
				dz[c] = g * (sg * (1.0f - sg));
			}
#pragma unroll
			for (int c = 0; c < 3; c++) sc_dh(rw2, 3 * j + c, dz[c], dh);
			row++;
		}
#pragma unroll
		for (int c = 0; c < 3; c++) st[(size_t)(R.o_col + 3 * j + c) * cap] = dz[c];
	}
	for (int o = 3 * K; o < R.p3; o++) st[(size_t)(R.o_col + o) * cap] = 0.0f;
	sc_hidden_bwd<SC_IN>(rw1, h, dh, hl, dx, st + (size_t)R.o_dcol * cap, sr + (size_t)(2 * SC_FEAT) * cap, cap);

	// dx -> anchor_feat and (view, dist)
	float dvd[4] = {dx[SC_FEAT], dx[SC_FEAT + 1], dx[SC_FEAT + 2], dx[SC_FEAT + 3]};
	float4* dfp = reinterpret_cast<float4*>(d_feat + (size_t)a * SC_FEAT);
	if (!BANK) {
#pragma unroll
		for (int i = 0; i < SC_FEAT / 4; i++) dfp[i] = make_float4(dx[4 * i], dx[4 * i + 1], dx[4 * i + 2], dx[4 * i + 3]);
	} else {
		float f[SC_FEAT], w[3];
		const float4* fp = reinterpret_cast<const float4*>(feat + (size_t)a * SC_FEAT);
#pragma unroll
		for (int i = 0; i < SC_FEAT / 4; i++) {
			const float4 v = fp[i];
			f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
		}
		sc_bank_w(kw1, kb1, kw2, kb2, x + SC_FEAT, hl, h, w);   // h = the bank's hidden layer
		// the transpose of x[c] = f[4 (c % 8)] w0 + f[2 (c % 16)] w1 + f[c] w2
		float dw0 = 0.0f, dw1 = 0.0f, dw2 = 0.0f, df[SC_FEAT];
#pragma unroll
		for (int c = 0; c < SC_FEAT; c++) {
			dw0 = FMA(dx[c], f[4 * (c % 8)], dw0);
			dw1 = FMA(dx[c], f[2 * (c % 16)], dw1);
			dw2 = FMA(dx[c], f[c], dw2);
			df[c] = dx[c] * w[2];
		}
#pragma unroll
		for (int c = 0; c < SC_FEAT; c++) df[2 * (c % 16)] = FMA(dx[c], w[1], df[2 * (c % 16)]);
#pragma unroll
		for (int c = 0; c < SC_FEAT; c++) df[4 * (c % 8)] = FMA(dx[c], w[0], df[4 * (c % 8)]);
#pragma unroll
		for (int i = 0; i < SC_FEAT / 4; i++) dfp[i] = make_float4(df[4 * i], df[4 * i + 1], df[4 * i + 2], df[4 * i + 3]);
		// softmax: do = w (dw - sum w dw)
		const float dot = FMA(w[2], dw2, FMA(w[1], dw1, w[0] * dw0));
		const float dob[3] = {w[0] * (dw0 - dot), w[1] * (dw1 - dot), w[2] * (dw2 - dot)};
#pragma unroll
		for (int i = 0; i < SC_FEAT; i++) dh[i] = 0.0f;
#pragma unroll
		for (int o = 0; o < 3; o++) {
			sc_dh(kw2, o, dob[o], dh);
			st[(size_t)(R.o_bank + o) * cap] = dob[o];
		}
		st[(size_t)(R.o_bank + 3) * cap] = 0.0f;
		sc_hidden_bwd<4>(kw1, h, dh, hl, dvd, st + (size_t)R.o_dbank * cap, sr + (size_t)(3 * SC_FEAT + SC_IN) * cap, cap);
	}
	// view = v / d, dist = d: dv = (dview - view (view . dview)) / d + ddist view
	const float d = x[SC_FEAT + 3];
	const float t = FMA(x[SC_FEAT + 2], dvd[2], FMA(x[SC_FEAT + 1], dvd[1], x[SC_FEAT] * dvd[0]));
	const float dv0 = (dvd[0] - x[SC_FEAT] * t) / d + dvd[3] * x[SC_FEAT];
	const float dv1 = (dvd[1] - x[SC_FEAT + 1] * t) / d + dvd[3] * x[SC_FEAT + 1];
	const float dv2 = (dvd[2] - x[SC_FEAT + 2] * t) / d + dvd[3] * x[SC_FEAT + 2];
	d_anchor[3 * (size_t)a] = ga0 + dv0;
	d_anchor[3 * (size_t)a + 1] = ga1 + dv1;
	d_anchor[3 * (size_t)a + 2] = ga2 + dv2;
#pragma unroll
	for (int i = 0; i < 6; i++) d_scaling[6 * (size_t)a + i] = ds6[i];
}

// the right-vector slot of left row `row`
__device__ __forceinline__ int sc_row_slot(int row, const ScRows& R)
{
	if (row < R.o_dop) return 0;
	if (row < R.o_cov) return 3;
	if (row < R.o_dcov) return 1;
	if (row < R.o_col) return 3;
	if (row < R.o_dcol) return 2;
	if (row < R.o_bank) return 3;
	if (row < R.o_dbank) return 4;
	return 5;
}

// grid (blocks of this chunk = chains, slices of the row space).  Thread id = slice * 256 + t owns rows 4 (id / 5) .. + 3 and
// columns 8 (id % 5) .. + 7 of the chain's partial sums [lpad][SB_SLOT].
__global__ void __launch_bounds__(256) scaffold_bwd_wsum(int N, int K, int M, int bank, int block0, size_t cap,
                                                         const float* __restrict__ stage, const unsigned short* __restrict__ kept,
                                                         const int* __restrict__ start, float* __restrict__ partials, int first)
{
	__shared__ __attribute__((aligned(16))) float s[SB_TILE * SB_STRIDE];
	const ScRows R = sc_rows(K, bank != 0);
	const int tid = threadIdx.x;
	const int id = blockIdx.y * 256 + tid;
	const int rg = id / 5, cg = id % 5;
	const bool active = 4 * rg < R.lpad;
	const int row_lo = 4 * ((blockIdx.y * 256) / 5);
	const int nrows = min(SB_LROWS, R.lpad - row_lo);
	const int nright = bank ? SB_RIGHT : SB_RIGHT - SC_FEAT;
	const int chain = blockIdx.x;   // block0 is a multiple of SB_CHAINS
	float* part = partials + ((size_t)chain * R.lpad + 4 * rg) * SB_SLOT + cg * 8;
	float acc[4][8];
#pragma unroll
	for (int r = 0; r < 4; r++)
#pragma unroll
		for (int c = 0; c < 8; c++) acc[r][c] = (first || !active) ? 0.0f : part[r * SB_SLOT + c];
	for (int i = tid; i < SB_TILE * SB_STRIDE; i += 256) s[i] = 0.0f;
	__syncthreads();
	if (tid < SB_TILE) {
		float* one = s + tid * SB_STRIDE + SB_LROWS;
		one[0 * SB_SLOT + SC_FEAT] = 1.0f;
		one[1 * SB_SLOT + SC_FEAT] = 1.0f;
		one[2 * SB_SLOT + SC_FEAT] = 1.0f;
		one[3 * SB_SLOT + SC_IN] = 1.0f;
		one[4 * SB_SLOT + SC_FEAT] = 1.0f;
		one[5 * SB_SLOT + 4] = 1.0f;
	}
	const int slot = sc_row_slot(4 * rg, R);
	const int al = tid & (SB_TILE - 1);
	for (int t = 0; t < 256 / SB_TILE; t++) {
		const int la = blockIdx.x * 256 + t * SB_TILE + al;       // index into the chunk's staging
		const int a = block0 * 256 + la;
		uint32_t kb = a < N ? kept[a] : 0;
		if (kb != 0) {
			const int s0 = start[a];
			if (s0 < 0 || (long long)s0 + __popc(kb) > (long long)M) kb = 0;
		}
		// every wave holds all SB_TILE anchors of the tile in its lanes: the same answer in every wave of the workgroup
		if (__ballot(kb != 0) == 0) continue;   // a tile without a kept anchor adds fma(0, 0, acc) = acc: skipped
		__syncthreads();
		for (int i = tid; i < (nrows + nright) * SB_TILE; i += 256) {   // i % SB_TILE == al
			const int v = i / SB_TILE;
			const int gv = v < nrows ? row_lo + v : R.lpad + (v - nrows);
			const float val = kb != 0 ? stage[(size_t)gv * cap + la] : 0.0f;
			float* sa = s + al * SB_STRIDE;
			if (v < nrows) {
				sa[v] = val;
			} else {
				const int r = v - nrows;
				if (r < 3 * SC_FEAT) {
					sa[SB_LROWS + (r / SC_FEAT) * SB_SLOT + (r % SC_FEAT)] = val;
				} else if (r < 3 * SC_FEAT + SC_IN) {
					sa[SB_LROWS + 3 * SB_SLOT + (r - 3 * SC_FEAT)] = val;
					if (r >= 4 * SC_FEAT) sa[SB_LROWS + 5 * SB_SLOT + (r - 4 * SC_FEAT)] = val;
				} else {
					sa[SB_LROWS + 4 * SB_SLOT + (r - 3 * SC_FEAT - SC_IN)] = val;
				}
			}
		}
		__syncthreads();
		if (active) {
			const float* lp = s + (4 * rg - row_lo);
			const float* rp = s + SB_LROWS + slot * SB_SLOT + cg * 8;
#pragma unroll 2
			for (int n = 0; n < SB_TILE; n++) {
				const float4 l4 = *reinterpret_cast<const float4*>(lp + n * SB_STRIDE);
				const float4 ra = *reinterpret_cast<const float4*>(rp + n * SB_STRIDE);
				const float4 rb = *reinterpret_cast<const float4*>(rp + n * SB_STRIDE + 4);
				const float l[4] = {l4.x, l4.y, l4.z, l4.w};
				const float rv[8] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};
#pragma unroll
				for (int r = 0; r < 4; r++)
#pragma unroll
					for (int c = 0; c < 8; c++) acc[r][c] = FMA(l[r], rv[c], acc[r][c]);
			}
		}
	}
	if (active) {
#pragma unroll
		for (int r = 0; r < 4; r++)
#pragma unroll
			for (int c = 0; c < 8; c++) part[r * SB_SLOT + c] = acc[r][c];
	}
}

struct ScGradPtrs {
	float* p[16];
};

// one thread per (row, column) of the row space: the chains' partials in ascending chain order, in float64
__global__ void __launch_bounds__(256) scaffold_bwd_final(int K, int bank, int nch, const float* __restrict__ partials, ScGradPtrs out)
{
	const ScRows R = sc_rows(K, bank != 0);
	const int idx = blockIdx.x * 256 + threadIdx.x;
	if (idx >= R.lpad * SB_SLOT) return;
	const int row = idx / SB_SLOT, col = idx % SB_SLOT;
	int mlp, o, nout, nin;
	bool second;   // W2 / b2 (left = dout) or W1 / b1 (left = dpre)
	if (row < R.o_dop) { mlp = 0; second = true; o = row; nout = K; }
	else if (row < R.o_cov) { mlp = 0; second = false; o = row - R.o_dop; nout = SC_FEAT; }
	else if (row < R.o_dcov) { mlp = 1; second = true; o = row - R.o_cov; nout = 7 * K; }
	else if (row < R.o_col) { mlp = 1; second = false; o = row - R.o_dcov; nout = SC_FEAT; }
	else if (row < R.o_dcol) { mlp = 2; second = true; o = row - R.o_col; nout = 3 * K; }
	else if (row < R.o_bank) { mlp = 2; second = false; o = row - R.o_dcol; nout = SC_FEAT; }
	else if (row < R.o_dbank) { mlp = 3; second = true; o = row - R.o_bank; nout = 3; }
	else { mlp = 3; second = false; o = row - R.o_dbank; nout = SC_FEAT; }
	nin = second ? SC_FEAT : (mlp == 3 ? 4 : SC_IN);
	if (o >= nout || col > nin) return;
	double sum = 0.0;
	for (int c = 0; c < nch; c++) sum += (double)partials[((size_t)c * R.lpad + row) * SB_SLOT + col];
	const float v = (float)sum;
	float* w = out.p[4 * mlp + (second ? 2 : 0)];
	float* b = out.p[4 * mlp + (second ? 3 : 1)];
	if (col < nin) w[o * nin + col] = v;
	else b[o] = v;
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

int gsr_scaffold_backward(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* anchor, const float* anchor_feat,
                          const float* offset, const float* scaling, const float* const weights[16], int num_anchors, int n_offsets,
                          const float* campos, const unsigned short* kept, const int* start, int num_gaussians, const float* g_xyz,
                          const float* g_colors, const float* g_opacity, const float* g_scales, const float* g_rotations,
                          float* d_anchor, float* d_anchor_feat, float* d_offset, float* d_scaling, float* const d_weights[16],
                          void* stream)
{
	const int N = num_anchors, K = n_offsets, M = num_gaussians;
	if (!sc_sizes_ok(N, K) || !weights || !d_weights || !campos || M < 0 || (long long)M > (long long)N * K) return GSR_ERR_ARG;
	for (int i = 0; i < 12; i++)
		if (!weights[i] || !d_weights[i]) return GSR_ERR_ARG;
	const bool bank = weights[12] != nullptr;
	for (int i = 12; i < 16; i++)
		if (bank && (!weights[i] || !d_weights[i])) return GSR_ERR_ARG;
	if (N > 0 && (!d_anchor || !d_anchor_feat || !d_offset || !d_scaling)) return GSR_ERR_ARG;
	if (M > 0 && (!anchor || !anchor_feat || !offset || !scaling || !kept || !start)) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	// the per-anchor outputs are pre-zeroed: scaffold_bwd_anchor writes the rows of anchors with a kept offset only
	if (N > 0) {
		GSR_TRY(hipMemsetAsync(d_anchor, 0, sizeof(float) * 3 * (size_t)N, s));
		GSR_TRY(hipMemsetAsync(d_anchor_feat, 0, sizeof(float) * SC_FEAT * (size_t)N, s));
		GSR_TRY(hipMemsetAsync(d_offset, 0, sizeof(float) * 3 * (size_t)N * K, s));
		GSR_TRY(hipMemsetAsync(d_scaling, 0, sizeof(float) * 6 * (size_t)N, s));
	}
	if (M == 0) {   // no kernel: every gradient is zero
		const int nout[4] = {K, 7 * K, 3 * K, 3}, nin[4] = {SC_IN, SC_IN, SC_IN, 4};
		for (int m = 0; m < (bank ? 4 : 3); m++) {
			GSR_TRY(hipMemsetAsync(d_weights[4 * m], 0, sizeof(float) * SC_FEAT * nin[m], s));
			GSR_TRY(hipMemsetAsync(d_weights[4 * m + 1], 0, sizeof(float) * SC_FEAT, s));
			GSR_TRY(hipMemsetAsync(d_weights[4 * m + 2], 0, sizeof(float) * SC_FEAT * nout[m], s));
			GSR_TRY(hipMemsetAsync(d_weights[4 * m + 3], 0, sizeof(float) * nout[m], s));
		}
		return GSR_OK;
	}
	const ScRows R = sc_rows(K, bank);
	const int nblocks = (int)blocks(N);
	const int nch = nblocks < SB_CHAINS ? nblocks : SB_CHAINS;
	const size_t cap = (size_t)nch * 256;   // anchors per chunk: at most 65536, whatever N is
	float *stage, *partials;
	auto carve = [&](Arena& ws) {
		stage = ws.take<float>((size_t)(R.lpad + SB_RIGHT) * cap);
		partials = ws.take<float>((size_t)nch * R.lpad * SB_SLOT);
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	const unsigned slices = (unsigned)((R.lpad / 4 * 5 + 255) / 256);
	auto kern = bank ? scaffold_bwd_anchor<true> : scaffold_bwd_anchor<false>;
	for (int block0 = 0; block0 < nblocks; block0 += SB_CHAINS) {
		const int nb = nblocks - block0 < SB_CHAINS ? nblocks - block0 : SB_CHAINS;
		hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, N, K, M, block0, cap, anchor, anchor_feat, offset, scaling, weights[0],
		                   weights[1], weights[2], weights[3], weights[4], weights[5], weights[6], weights[7], weights[8], weights[9],
		                   weights[10], weights[11], weights[12], weights[13], weights[14], weights[15], campos, kept, start, g_xyz,
		                   g_colors, g_opacity, g_scales, g_rotations, stage, d_anchor, d_anchor_feat, d_offset, d_scaling);
		hipLaunchKernelGGL(scaffold_bwd_wsum, dim3(nb, slices), dim3(256), 0, s, N, K, M, bank ? 1 : 0, block0, cap, stage, kept, start,
		                   partials, block0 == 0 ? 1 : 0);
	}
	ScGradPtrs out;
	for (int i = 0; i < 16; i++) out.p[i] = d_weights[i];
	hipLaunchKernelGGL(scaffold_bwd_final, dim3(blocks((long long)R.lpad * SB_SLOT)), dim3(256), 0, s, K, bank ? 1 : 0, nch, partials, out);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
