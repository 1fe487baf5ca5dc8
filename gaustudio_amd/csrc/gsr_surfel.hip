// gsr_surfel.hip -- the 2D Gaussian surfel ("2DGS") operator of libgsrast for gfx950 (MI355X, wave64).
//
//   surfel_preprocess_fwd   one lane per surfel: near-plane cull, splat-to-pixel matrix M, camera-facing normal,
//                           screen centre / extent / radius, the reference's square tile rect, SH -> RGB; writes the
//                           80-B SurfRec plus the 16-B binning record, tiles_touched and the block sums in the formats the
//                           3DGS binning, scan and sort launchers consume (they run unchanged on a surfel frame)
//   surfel_composite_fwd    one workgroup per 16x16 tile, one pixel per lane, records staged through LDS planes (SoA);
//                           front-to-back ray-splat intersection and compositing -> colour and the 7-channel allmap
//   surfel_composite_bwd    the same walk again (same decisions: the forward's contributor count bounds it), exact
//                           derivative per (pixel, surfel), reduced over the tile in a fixed order into ONE 64-B row per
//                           (tile, surfel) instance in the Gaussian-major goff order -- no atomics
//   surfel_preprocess_bwd   one lane per surfel: sums its rows in ascending order, then M -> (mean, scales, rotation),
//                           normal -> rotation, the means2D densification proxy; the SH backward is the 3DGS one
//
// Semantics (constants: gsr_common.h GSR_SURF_*; restated in float64 by tests/surfel_model.py):
//   X(u, v) = p + u s_u t_u + v s_v t_v,  h = (c.x W/2 + c.w (W-1)/2, c.y H/2 + c.w (H-1)/2, c.w) = M (u, v, 1),  c = proj X
//   pixel (x, y): k = x Tw - Tu, l = y Tw - Tv, q = k x l, (u, v) = q.xy / q.z, rho = min(u^2 + v^2, 2 |centre - (x, y)|^2)
#include "gsr_internal.h"

namespace gsr {

__device__ __constant__ float sSH_C0 = 0.28209479177387814f;
__device__ __constant__ float sSH_C1 = 0.4886025119029199f;
__device__ __constant__ float sSH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                            -1.0925484305920792f, 0.5462742152960396f};
__device__ __constant__ float sSH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                            0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                            -0.5900435899266435f};

// Q = ndc2pix * proj: pixel-homogeneous h = Q (X, 1) for a world point X (rows 0, 1, 2 = h.x, h.y, h.w)
__device__ __forceinline__ void surf_q(const float* proj, int W, int H, float Q[3][4])
{
	const float hw = 0.5f * (float)W, hh = 0.5f * (float)H, ow = 0.5f * (float)(W - 1), oh = 0.5f * (float)(H - 1);
#pragma unroll
	for (int k = 0; k < 4; k++) {
		Q[0][k] = FMA(hw, proj[4 * k + 0], ow * proj[4 * k + 3]);
		Q[1][k] = FMA(hh, proj[4 * k + 1], oh * proj[4 * k + 3]);
		Q[2][k] = proj[4 * k + 3];
	}
}

// The per-(pixel, surfel) evaluation shared by both compositing kernels: the same operations in the same order, so that
// the backward takes every decision the forward took.  Returns false when the surfel is skipped at this pixel.
struct SurfHit {
	float kx, ky, kz, lx, ly, lz, qz, u, v, z, G, alpha;
	bool in3;      // rho3 <= rho2: the ray-splat intersection (else the low-pass branch)
	bool clamped;  // o G > ALPHA_MAX
};
__device__ __forceinline__ bool surf_eval(const float* Tu, const float* Tv, const float* Tw, float cx, float cy, float o, float px,
                                          float py, bool fx, SurfHit& h)
{
	h.kx = px * Tw[0] - Tu[0]; h.ky = px * Tw[1] - Tu[1]; h.kz = px * Tw[2] - Tu[2];
	h.lx = py * Tw[0] - Tv[0]; h.ly = py * Tw[1] - Tv[1]; h.lz = py * Tw[2] - Tv[2];
	const float qx = h.ky * h.lz - h.kz * h.ly;
	const float qy = h.kz * h.lx - h.kx * h.lz;
	h.qz = h.kx * h.ly - h.ky * h.lx;
	if (h.qz == 0.0f) return false;
	h.u = qx / h.qz;
	h.v = qy / h.qz;
	const float rho3 = h.u * h.u + h.v * h.v;
	const float dx = cx - px, dy = cy - py;
	const float rho2 = GSR_SURF_LOWPASS * (dx * dx + dy * dy);
	h.in3 = rho3 <= rho2;
	const float rho = h.in3 ? rho3 : rho2;
	h.z = h.in3 ? (h.u * Tw[0] + h.v * Tw[1]) + Tw[2] : Tw[2];
	if (h.z < GSR_SURF_NEAR) return false;
	// exp's argument clamped to the domain of gs_exp: o exp(-80) < 1/255 for any opacity <= 1, the decision is unchanged
	const float pw = fmaxf(-0.5f * rho, -80.0f);
	h.G = fx ? gs_exp_hw(pw) : gs_exp(pw);
	const float a = o * h.G;
	h.clamped = a > GSR_SURF_ALPHA_MAX;
	h.alpha = fminf(GSR_SURF_ALPHA_MAX, a);
	return !(h.alpha < GSR_SURF_ALPHA_MIN);
}

// m = FAR / (FAR - NEAR) * (1 - NEAR / z): the normalised depth of the distortion loss
__device__ __forceinline__ float surf_m(float z) { return (GSR_SURF_FAR / (GSR_SURF_FAR - GSR_SURF_NEAR)) * (1.0f - GSR_SURF_NEAR / z); }

// ------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void surfel_preprocess_fwd_kernel(
    int P, int M, const float* __restrict__ means3D, const float* __restrict__ scales, float scale_modifier,
    const float* __restrict__ rotations, const float* __restrict__ opacities, const float* __restrict__ shs,
    const float* __restrict__ colors_precomp, const GsCam* __restrict__ cam, int W, int H, int gx, int gy,
    int* __restrict__ radii, SurfRec* __restrict__ recs, float* __restrict__ shjac, uint4* __restrict__ binfo,
    uint32_t* __restrict__ tiles_touched, uint32_t* __restrict__ bsums, uint32_t* __restrict__ refsums)
{
	constexpr int NC = (D + 1) * (D + 1);
	const int idx = blockIdx.x * 256 + threadIdx.x;
	uint32_t my_tiles = 0;
	if (idx < P) {
		int rad = 0;
		do {
			const float* view = cam->view;
			const float3 p = {means3D[3 * idx], means3D[3 * idx + 1], means3D[3 * idx + 2]};
			const float3 pv = xform4x3(p, view);
			if (pv.z <= GSR_SURF_NEAR) break;
			float inv_len;
			const float4 q = gs_act_rot(*reinterpret_cast<const float4*>(rotations + 4 * (size_t)idx), GSR_ACT_ROT_NORMALIZE, &inv_len);
			const M3 R = quat_to_R(q);   // R.m[c] = column c: t_u, t_v, t_n
			const float su = scale_modifier * scales[2 * idx], sv = scale_modifier * scales[2 * idx + 1];
			float Q[3][4];
			surf_q(cam->proj, W, H, Q);
			float Mm[3][3];   // Mm[row][col]
#pragma unroll
			for (int r = 0; r < 3; r++) {
				const float a = FMA(Q[r][2], R.m[0][2], FMA(Q[r][1], R.m[0][1], Q[r][0] * R.m[0][0]));
				const float b = FMA(Q[r][2], R.m[1][2], FMA(Q[r][1], R.m[1][1], Q[r][0] * R.m[1][0]));
				Mm[r][0] = a * su;
				Mm[r][1] = b * sv;
				Mm[r][2] = FMA(Q[r][2], p.z, FMA(Q[r][1], p.y, Q[r][0] * p.x)) + Q[r][3];
			}
			// view-space normal, flipped towards the camera
			float3 n;
			n.x = FMA(view[8], R.m[2][2], FMA(view[4], R.m[2][1], view[0] * R.m[2][0]));
			n.y = FMA(view[9], R.m[2][2], FMA(view[5], R.m[2][1], view[1] * R.m[2][0]));
			n.z = FMA(view[10], R.m[2][2], FMA(view[6], R.m[2][1], view[2] * R.m[2][0]));
			const float cosv = -FMA(pv.z, n.z, FMA(pv.y, n.y, pv.x * n.x));
			if (cosv == 0.0f) break;
			const float sgn = cosv > 0.0f ? 1.0f : -1.0f;
			n.x *= sgn; n.y *= sgn; n.z *= sgn;
			// centre and extent of the 3-sigma footprint
			const float c2 = GSR_SURF_CUTOFF * GSR_SURF_CUTOFF;
			const float dist = FMA(c2, Mm[2][1] * Mm[2][1], c2 * (Mm[2][0] * Mm[2][0])) - Mm[2][2] * Mm[2][2];
			if (dist == 0.0f) break;
			const float fx = c2 / dist, fz = -1.0f / dist;
			const float cx = FMA(fz, Mm[0][2] * Mm[2][2], FMA(fx, Mm[0][1] * Mm[2][1], fx * (Mm[0][0] * Mm[2][0])));
			const float cy = FMA(fz, Mm[1][2] * Mm[2][2], FMA(fx, Mm[1][1] * Mm[2][1], fx * (Mm[1][0] * Mm[2][0])));
			const float tx = FMA(fz, Mm[0][2] * Mm[0][2], FMA(fx, Mm[0][1] * Mm[0][1], fx * (Mm[0][0] * Mm[0][0])));
			const float ty = FMA(fz, Mm[1][2] * Mm[1][2], FMA(fx, Mm[1][1] * Mm[1][1], fx * (Mm[1][0] * Mm[1][0])));
			const float ex = sqrtf(fmaxf(1e-4f, cx * cx - tx)), ey = sqrtf(fmaxf(1e-4f, cy * cy - ty));
			const float my_radius = ceilf(fmaxf(fmaxf(ex, ey), GSR_SURF_MIN_EXTENT));
			// getRect (the reference's square), exactly as preprocess_fwd forms it
			const int r_ = (int)my_radius;
			const int rminx = min(gx, max(0, (int)((cx - r_) / GSR_BLOCK_X)));
			const int rminy = min(gy, max(0, (int)((cy - r_) / GSR_BLOCK_Y)));
			const int rmaxx = min(gx, max(0, (int)((cx + r_ + GSR_BLOCK_X - 1) / GSR_BLOCK_X)));
			const int rmaxy = min(gy, max(0, (int)((cy + r_ + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y)));
			if ((rmaxx - rminx) * (rmaxy - rminy) == 0) break;
			float rgb[3];
			uint32_t clamped = 0;
			if (colors_precomp == nullptr) {
				float sh[NC * 3];
				const float* shp = shs + (size_t)idx * M * 3;
#pragma unroll
				for (int i = 0; i < NC * 3; i++) sh[i] = shp[i];
				float3 dir = {p.x - cam->campos[0], p.y - cam->campos[1], p.z - cam->campos[2]};
				const float len = sqrtf(FMA(dir.z, dir.z, FMA(dir.y, dir.y, dir.x * dir.x)));
				dir.x = dir.x / len; dir.y = dir.y / len; dir.z = dir.z / len;
				clamped = gs_sh_eval<D>(sSH_C0, sSH_C1, sSH_C2, sSH_C3, sh, dir.x, dir.y, dir.z, rgb);
				if (D > 0) {
					// d(rgb) / d(view direction) for the (3DGS) SH backward, exactly as preprocess_fwd leaves it
					float J[9];
					gs_sh_dir_jacobian<D>(sSH_C1, sSH_C2, sSH_C3, sh, dir.x, dir.y, dir.z, J);
#pragma unroll
					for (int k = 0; k < 9; k++) shjac[9 * (size_t)idx + k] = J[k];
				}
			} else {
				rgb[0] = colors_precomp[3 * (size_t)idx];
				rgb[1] = colors_precomp[3 * (size_t)idx + 1];
				rgb[2] = colors_precomp[3 * (size_t)idx + 2];
			}
			SurfRec rec;
			rec.q0 = make_float4(Mm[0][0], Mm[0][1], Mm[0][2], Mm[1][0]);
			rec.q1 = make_float4(Mm[1][1], Mm[1][2], Mm[2][0], Mm[2][1]);
			rec.q2 = make_float4(Mm[2][2], cx, cy, opacities[idx]);
			rec.q3 = make_float4(n.x, n.y, n.z, my_radius);
			rec.q4 = make_float4(rgb[0], rgb[1], rgb[2], sgn);
			recs[idx] = rec;
			// the 16-B binning record of the 3DGS path: rect, clamp bits (no dead corners), depth bits (> NEAR: order as uint)
			binfo[idx] = make_uint4((uint32_t)rminx | ((uint32_t)rminy << 16), (uint32_t)rmaxx | ((uint32_t)rmaxy << 16), clamped,
			                        (uint32_t)__float_as_int(pv.z));
			my_tiles = (uint32_t)((rmaxx - rminx) * (rmaxy - rminy));
			rad = r_;
		} while (0);
		radii[idx] = rad;
		tiles_touched[idx] = my_tiles;
	}
	// per-256-block sums of the binned tiles (tile_scan's second workgroup scans them into the goff bases); the binned rects
	// ARE the reference's squares here, so both sums are the same
	__shared__ uint32_t s_sum[4];
	uint32_t a = my_tiles;
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) a += (uint32_t)__shfl_xor((int)a, o, 64);
	if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = a;
	__syncthreads();
	if (threadIdx.x == 0) {
		const uint32_t t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
		bsums[blockIdx.x] = t;
		refsums[blockIdx.x] = t;
	}
}

void launch_surfel_preprocess_fwd(const SurfFwdArgs& a, const GsCam* cam, const ImgLayout& il, int* radii, SurfRec* recs, float* shjac,
                                  uint4* binfo, uint32_t* tiles_touched, uint32_t* bsums, uint32_t* refsums, hipStream_t s)
{
	const int D = a.colors_precomp ? 0 : a.D;
	dim3 grid((a.P + 255) / 256), block(256);
#define GSR_LAUNCH_SPRE(DEG)                                                                                              \
	hipLaunchKernelGGL((surfel_preprocess_fwd_kernel<DEG>), grid, block, 0, s, a.P, a.M, a.means3D, a.scales, a.scale_modifier, \
	                   a.rotations, a.opacities, a.shs, a.colors_precomp, cam, a.W, a.H, il.gx, il.gy, radii, recs, shjac, binfo, \
	                   tiles_touched, bsums, refsums)
	switch (D) {
		case 0: GSR_LAUNCH_SPRE(0); break;
		case 1: GSR_LAUNCH_SPRE(1); break;
		case 2: GSR_LAUNCH_SPRE(2); break;
		default: GSR_LAUNCH_SPRE(3); break;
	}
#undef GSR_LAUNCH_SPRE
}

// ------------------------------------------------------------------------------------------------
// Records of a batch of 256 list entries in LDS, one plane per field (structure of arrays): in the walk every lane reads the
// same entry (a broadcast), the staging store of lane t goes to word t of each plane -- neither side has bank conflicts.
#define SP_TU 0
#define SP_TV 3
#define SP_TW 6
#define SP_CX 9
#define SP_CY 10
#define SP_OP 11
#define SP_N 12
#define SP_RGB 15
#define SP_FWD_PLANES 18
#define SP_BWD_PLANES 19   // + the entry's row index (as float bits)
__device__ __forceinline__ void surf_stage(float (*pl)[256], int t, const SurfRec& r)
{
	pl[SP_TU + 0][t] = r.q0.x; pl[SP_TU + 1][t] = r.q0.y; pl[SP_TU + 2][t] = r.q0.z;
	pl[SP_TV + 0][t] = r.q0.w; pl[SP_TV + 1][t] = r.q1.x; pl[SP_TV + 2][t] = r.q1.y;
	pl[SP_TW + 0][t] = r.q1.z; pl[SP_TW + 1][t] = r.q1.w; pl[SP_TW + 2][t] = r.q2.x;
	pl[SP_CX][t] = r.q2.y; pl[SP_CY][t] = r.q2.z; pl[SP_OP][t] = r.q2.w;
	pl[SP_N + 0][t] = r.q3.x; pl[SP_N + 1][t] = r.q3.y; pl[SP_N + 2][t] = r.q3.z;
	pl[SP_RGB + 0][t] = r.q4.x; pl[SP_RGB + 1][t] = r.q4.y; pl[SP_RGB + 2][t] = r.q4.z;
}

template <bool FX>
__global__ __launch_bounds__(256) void surfel_composite_fwd_kernel(int W, int H, int gx, const uint2* __restrict__ ranges,
                                                                   const uint32_t* __restrict__ point_list,
                                                                   const SurfRec* __restrict__ recs, const GsCam* __restrict__ cam,
                                                                   float* __restrict__ out_color, float* __restrict__ out_allmap,
                                                                   float* __restrict__ final_T, uint32_t* __restrict__ n_contrib,
                                                                   uint32_t* __restrict__ med_pos, float* __restrict__ m1_out,
                                                                   float* __restrict__ m2_out, float* __restrict__ m0_out)
{
	__shared__ float pl[SP_FWD_PLANES][256];
	const int tile = blockIdx.x, tid = threadIdx.x;
	int lx, ly;
	gs_pixel_of_thread(tid, lx, ly);
	const int ix = (tile % gx) * GSR_BLOCK_X + lx, iy = (tile / gx) * GSR_BLOCK_Y + ly;
	const bool inside = ix < W && iy < H;
	const float px = (float)ix, py = (float)iy;
	const uint2 range = ranges[tile];
	// M1 / M2 are the moments of m - mref, mref = m of the pixel's first contributor: the distortion is invariant under a shift of
	// m, and m = FAR / (FAR - NEAR) (1 - NEAR / z) lies within a few per cent of 1 -- unshifted, every term cancels to ~1e-4 of its size
	float T = 1.0f, C[3] = {0.f, 0.f, 0.f}, Nn[3] = {0.f, 0.f, 0.f}, Dd = 0.f, M1 = 0.f, M2 = 0.f, dist = 0.f, median = 0.f, mref = 0.f;
	uint32_t contributor = 0, last = 0, medp = 0;
	bool done = !inside;
	for (uint32_t base = range.x; base < range.y; base += 256) {
		if (__syncthreads_count(done) == 256) break;   // (also the barrier before the planes are overwritten)
		const uint32_t j = base + (uint32_t)tid;
		if (j < range.y) surf_stage(pl, tid, recs[point_list[j]]);
		__syncthreads();
		const int cnt = (int)min(256u, range.y - base);
		for (int e = 0; !done && e < cnt; e++) {
			contributor++;
			const float Tu[3] = {pl[SP_TU][e], pl[SP_TU + 1][e], pl[SP_TU + 2][e]};
			const float Tv[3] = {pl[SP_TV][e], pl[SP_TV + 1][e], pl[SP_TV + 2][e]};
			const float Tw[3] = {pl[SP_TW][e], pl[SP_TW + 1][e], pl[SP_TW + 2][e]};
			SurfHit h;
			if (!surf_eval(Tu, Tv, Tw, pl[SP_CX][e], pl[SP_CY][e], pl[SP_OP][e], px, py, FX, h)) continue;
			const float test_T = T * (1.0f - h.alpha);
			if (test_T < GSR_SURF_T_MIN) { done = true; break; }
			const float w = h.alpha * T;
			if (last == 0) mref = surf_m(h.z);
			const float m = surf_m(h.z) - mref;
			dist += w * (((m * m) * (1.0f - T) + M2) - (2.0f * m) * M1);
			Dd += w * h.z;
			M1 += w * m;
			M2 += w * (m * m);
#pragma unroll
			for (int c = 0; c < 3; c++) {
				Nn[c] += w * pl[SP_N + c][e];
				C[c] += w * pl[SP_RGB + c][e];
			}
			if (T > GSR_SURF_MEDIAN_T) { median = h.z; medp = contributor; }
			T = test_T;
			last = contributor;
		}
	}
	if (!inside) return;
	const size_t HW = (size_t)W * H, pix = (size_t)W * iy + ix, slot = (size_t)tile * GSR_TILE_PIX + tid;
	final_T[slot] = T;
	n_contrib[slot] = last;
	med_pos[slot] = medp;
	m1_out[slot] = M1;
	m2_out[slot] = M2;
	m0_out[slot] = mref;
#pragma unroll
	for (int c = 0; c < 3; c++) out_color[c * HW + pix] = C[c] + T * cam->bg[c];
	out_allmap[pix] = Dd;
	out_allmap[HW + pix] = 1.0f - T;
	out_allmap[2 * HW + pix] = Nn[0];
	out_allmap[3 * HW + pix] = Nn[1];
	out_allmap[4 * HW + pix] = Nn[2];
	out_allmap[5 * HW + pix] = median;
	out_allmap[6 * HW + pix] = dist;
}

void launch_surfel_composite_fwd(const ImgLayout& il, int W, int H, const uint2* ranges, const uint32_t* point_list, const SurfRec* recs,
                                 const GsCam* cam, float* out_color, float* out_allmap, float* final_T, uint32_t* n_contrib,
                                 uint32_t* med_pos, float* m1, float* m2, float* m0, bool fast_exp, hipStream_t s)
{
	if (fast_exp)
		hipLaunchKernelGGL(surfel_composite_fwd_kernel<true>, dim3(il.T), dim3(256), 0, s, W, H, il.gx, ranges, point_list, recs, cam,
		                   out_color, out_allmap, final_T, n_contrib, med_pos, m1, m2, m0);
	else
		hipLaunchKernelGGL(surfel_composite_fwd_kernel<false>, dim3(il.T), dim3(256), 0, s, W, H, il.gx, ranges, point_list, recs, cam,
		                   out_color, out_allmap, final_T, n_contrib, med_pos, m1, m2, m0);
}

// ------------------------------------------------------------------------------------------------
// Backward walk, BACK TO FRONT, from the tile's last contributor to the first entry.  For entry i of a pixel (T_i before it,
// w_i = alpha_i T_i) and an output O = sum w_j f_j (+ T_f bg):
//   dO/df_i = w_i,   dO/dalpha_i = T_i (f_i - R_{i+1}),   R_i = alpha_i f_i + (1 - alpha_i) R_{i+1},   R_{last+1} = bg (colour) or 0
// R_{i+1} is what lies behind entry i, per unit of the transmittance that reaches it: a convex combination, accumulated
// directly.  (Formed as the forward's total minus the running prefix -- two O(1) numbers that carry the rounding of every
// addition -- the remainder loses its relative accuracy as T_i falls towards 1e-4: an absolute error of ~1e-6 on the dL/dalpha
// of entries deep in a list of a thousand, tests/test_gpu_surfel_edges.py test_long_lists.)  T_i = T_{i+1} / (1 - alpha_i)
// from the forward's final T.  The distortion dist = sum_{j<i} w_i w_j (m_i - m_j)^2 has
//   g_i = ddist/dw_i = m_i^2 A_f + M2_f - 2 m_i M1_f,   ddist/dm_i = 2 w_i (m_i A_f - M1_f),   sum_j w_j g_j = 2 dist
// (A_f = 1 - T_f, M1_f, M2_f: the pixel's final values, kept by the forward, moments of m - mref).  Every decision is the forward's (surf_eval),
// the walk starts at the forward's last contributor.  Per entry the 16 partials are summed over the wave (butterfly) and then
// over the four waves in a fixed order: the row is bit-identical from run to run.
#define SURF_CHUNK 32   // entries per LDS reduction round
template <bool FX>
__global__ __launch_bounds__(256) void surfel_composite_bwd_kernel(
    int W, int H, int gx, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, const SurfRec* __restrict__ recs,
    const uint4* __restrict__ binfo, const uint32_t* __restrict__ goff, const float* __restrict__ final_T,
    const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ med_pos, const float* __restrict__ m1_in,
    const float* __restrict__ m2_in, const float* __restrict__ m0_in, const GsCam* __restrict__ cam,
    const float* __restrict__ dL_dcolor, const float* __restrict__ dL_dallmap, float* __restrict__ rows)
{
	__shared__ float pl[SP_BWD_PLANES][256];
	__shared__ float part[4][SURF_CHUNK][GSR_SURF_ROW];
	__shared__ uint32_t s_max;
	const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int tx = tile % gx, ty = tile / gx;
	int lx, ly;
	gs_pixel_of_thread(tid, lx, ly);
	const int ix = tx * GSR_BLOCK_X + lx, iy = ty * GSR_BLOCK_Y + ly;
	const bool inside = ix < W && iy < H;
	const float px = (float)ix, py = (float)iy;
	const uint2 range = ranges[tile];
	const size_t HW = (size_t)W * H, pix = inside ? (size_t)W * iy + ix : 0, slot = (size_t)tile * GSR_TILE_PIX + tid;
	const uint32_t last = inside ? n_contrib[slot] : 0u;
	if (tid == 0) s_max = 0u;
	__syncthreads();
	atomicMax(&s_max, last);   // (integer LDS max: order-independent)
	__syncthreads();
	const uint32_t walk = s_max;   // entries [0, walk) of the list have a contributor somewhere in the tile
	// upstream gradients (absent = zero) and the forward's totals
	float gC[3] = {0.f, 0.f, 0.f}, gN[3] = {0.f, 0.f, 0.f}, gD = 0.f, gA = 0.f, gMed = 0.f, gDist = 0.f;
	float Af = 0.f, M1f = 0.f, M2f = 0.f, mref = 0.f, T = 1.0f;
	uint32_t medp = 0;
	if (inside) {
		if (dL_dcolor != nullptr)
			for (int c = 0; c < 3; c++) gC[c] = dL_dcolor[c * HW + pix];
		if (dL_dallmap != nullptr) {
			gD = dL_dallmap[pix]; gA = dL_dallmap[HW + pix];
			for (int c = 0; c < 3; c++) gN[c] = dL_dallmap[(2 + c) * HW + pix];
			gMed = dL_dallmap[5 * HW + pix]; gDist = dL_dallmap[6 * HW + pix];
		}
		T = final_T[slot];   // T behind the pixel's last contributor
		Af = 1.0f - T;
		M1f = m1_in[slot];
		M2f = m2_in[slot];
		mref = m0_in[slot];
		medp = med_pos[slot];
	}
	// R_{i+1} of every composited quantity: colour (behind the last contributor: the background), normal, depth, alpha, ddist/dw
	float rC[3] = {cam->bg[0], cam->bg[1], cam->bg[2]}, rN[3] = {0.f, 0.f, 0.f}, rD = 0.f, rA = 0.f, rWG = 0.f;
	for (int b = (int)((walk + 255u) / 256u) - 1; b >= 0; b--) {
		const uint32_t base = range.x + 256u * (uint32_t)b;
		__syncthreads();   // the previous batch's planes are no longer read
		const uint32_t j = base + (uint32_t)tid;
		if (j < range.y) {
			const uint32_t g = point_list[j];
			surf_stage(pl, tid, recs[g]);
			const uint4 b = binfo[g];
			pl[SP_FWD_PLANES][tid] = __uint_as_float(goff[g] + gs_row_in_rect(b.x, b.y, 0u, tx, ty));
		}
		__syncthreads();
		const int cnt = (int)min(256u, range.x + walk - base);
		for (int c0 = ((cnt - 1) / SURF_CHUNK) * SURF_CHUNK; c0 >= 0; c0 -= SURF_CHUNK) {
			const int ce = min(SURF_CHUNK, cnt - c0);
			for (int el = ce - 1; el >= 0; el--) {
				const int e = c0 + el;
				const uint32_t contributor = 256u * (uint32_t)b + (uint32_t)e + 1u;   // the forward's 1-based list position
				float gr[GSR_SURF_ROW];
#pragma unroll
				for (int k = 0; k < GSR_SURF_ROW; k++) gr[k] = 0.f;
				bool act = false;
				if (contributor <= last) {
					const float Tu[3] = {pl[SP_TU][e], pl[SP_TU + 1][e], pl[SP_TU + 2][e]};
					const float Tv[3] = {pl[SP_TV][e], pl[SP_TV + 1][e], pl[SP_TV + 2][e]};
					const float Tw[3] = {pl[SP_TW][e], pl[SP_TW + 1][e], pl[SP_TW + 2][e]};
					const float o = pl[SP_OP][e];
					SurfHit h;
					if (surf_eval(Tu, Tv, Tw, pl[SP_CX][e], pl[SP_CY][e], o, px, py, FX, h)) {
						act = true;
						const float inv = 1.0f / (1.0f - h.alpha);
						T = T * inv;   // T_i, before this entry
						const float w = h.alpha * T;
						const float m = surf_m(h.z) - mref;   // (the forward's shift: g and ddist/dm are shift-invariant)
						const float n[3] = {pl[SP_N][e], pl[SP_N + 1][e], pl[SP_N + 2][e]};
						const float col[3] = {pl[SP_RGB][e], pl[SP_RGB + 1][e], pl[SP_RGB + 2][e]};
						const float gw = ((m * m) * Af + M2f) - (2.0f * m) * M1f;   // ddist / dw_i
						const float om = 1.0f - h.alpha;
						float dA = gA * (1.0f - rA) + gD * (h.z - rD) + gDist * (gw - rWG);
						for (int c = 0; c < 3; c++) {
							dA += gC[c] * (col[c] - rC[c]);
							dA += gN[c] * (n[c] - rN[c]);
							gr[10 + c] = w * gC[c];
							gr[13 + c] = w * gN[c];
							rC[c] = h.alpha * col[c] + om * rC[c];
							rN[c] = h.alpha * n[c] + om * rN[c];
						}
						dA *= T;
						rA = h.alpha + om * rA;
						rD = h.alpha * h.z + om * rD;
						rWG = h.alpha * gw + om * rWG;
						// dL/dz: expected depth, median (the forward's recorded contributor), distortion through m
						float dz = gD * w + gDist * (2.0f * w * (m * Af - M1f)) *
						                        ((GSR_SURF_FAR / (GSR_SURF_FAR - GSR_SURF_NEAR)) * GSR_SURF_NEAR / (h.z * h.z));
						if (contributor == medp) dz += gMed;
						float drho = 0.f;
						if (!h.clamped) {
							gr[9] = dA * h.G;
							drho = -0.5f * h.alpha * dA;
						}
						if (h.in3) {
							const float du = drho * 2.0f * h.u + dz * Tw[0];
							const float dv = drho * 2.0f * h.v + dz * Tw[1];
							gr[6] += dz * h.u;
							gr[7] += dz * h.v;
							gr[8] += dz;
							const float dqx = du / h.qz, dqy = dv / h.qz, dqz = -(du * h.u + dv * h.v) / h.qz;
							// q = k x l: dk = l x dq, dl = dq x k
							const float dkx = h.ly * dqz - h.lz * dqy, dky = h.lz * dqx - h.lx * dqz, dkz = h.lx * dqy - h.ly * dqx;
							const float dlx = dqy * h.kz - dqz * h.ky, dly = dqz * h.kx - dqx * h.kz, dlz = dqx * h.ky - dqy * h.kx;
							gr[0] = -dkx; gr[1] = -dky; gr[2] = -dkz;
							gr[3] = -dlx; gr[4] = -dly; gr[5] = -dlz;
							gr[6] += px * dkx + py * dlx;
							gr[7] += px * dky + py * dly;
							gr[8] += px * dkz + py * dlz;
						} else {
							gr[8] += dz;   // low-pass branch: z = Tw.z, the centre is not differentiated
						}
					}
				}
				if (__ballot(act) != 0ull) {
#pragma unroll
					for (int k = 0; k < GSR_SURF_ROW; k++) {
						float v = gr[k];
#pragma unroll
						for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
						gr[k] = v;
					}
				}
				if (lane < GSR_SURF_ROW) {
					float v = 0.f;
#pragma unroll
					for (int k = 0; k < GSR_SURF_ROW; k++) v = lane == k ? gr[k] : v;
					part[wv][el][lane] = v;
				}
			}
			__syncthreads();
			for (int i = tid; i < ce * GSR_SURF_ROW; i += 256) {
				const int el = i / GSR_SURF_ROW, k = i % GSR_SURF_ROW;
				const float v = ((part[0][el][k] + part[1][el][k]) + part[2][el][k]) + part[3][el][k];
				const uint32_t row = __float_as_uint(pl[SP_FWD_PLANES][c0 + el]);
				rows[(size_t)row * GSR_SURF_ROW + k] = v;
			}
			__syncthreads();
		}
	}
}

void launch_surfel_composite_bwd(const ImgLayout& il, int W, int H, const uint2* ranges, const uint32_t* point_list, const SurfRec* recs,
                                 const uint4* binfo, const uint32_t* goff, const float* final_T,
                                 const uint32_t* n_contrib, const uint32_t* med_pos, const float* m1, const float* m2, const float* m0,
                                 const GsCam* cam, const float* dL_dcolor, const float* dL_dallmap,
                                 float* rows, bool fast_exp, hipStream_t s)
{
	if (fast_exp)
		hipLaunchKernelGGL(surfel_composite_bwd_kernel<true>, dim3(il.T), dim3(256), 0, s, W, H, il.gx, ranges, point_list, recs, binfo,
		                   goff, final_T, n_contrib, med_pos, m1, m2, m0, cam, dL_dcolor, dL_dallmap, rows);
	else
		hipLaunchKernelGGL(surfel_composite_bwd_kernel<false>, dim3(il.T), dim3(256), 0, s, W, H, il.gx, ranges, point_list, recs, binfo,
		                   goff, final_T, n_contrib, med_pos, m1, m2, m0, cam, dL_dcolor, dL_dallmap, rows);
}

// ------------------------------------------------------------------------------------------------
// Per-surfel backward: the rows of the surfel summed in ascending order, then the chain rule through
//   M[:, 0] = Q3 (s_u t_u),  M[:, 1] = Q3 (s_v t_v),  M[:, 2] = Q3 p + Q[:, 3],  n = sgn R_view t_n,  (t_u t_v t_n) = R(q / |q|)
// and the densification proxy means2D.grad = (dL/dM02 M22 W/2, dL/dM12 M22 H/2, 0).  dL_dcolor gets the unmasked colour
// gradient; the SH stage of the 3DGS backward (launch_preprocess_bwd, GSR_PART_SH) turns it into dL_dsh afterwards.
__global__ __launch_bounds__(256) void surfel_preprocess_bwd_kernel(
    int P, int W, int H, const float* __restrict__ means3D, const float* __restrict__ scales, float scale_modifier,
    const float* __restrict__ rotations, const int* __restrict__ radii, const GsCam* __restrict__ cam, const SurfRec* __restrict__ recs,
    const uint32_t* __restrict__ goff, const float* __restrict__ rows, float* __restrict__ dL_dmean2D, float* __restrict__ dL_dopacity,
    float* __restrict__ dL_dcolor, float* __restrict__ dL_dmean3D, float* __restrict__ dL_dscale, float* __restrict__ dL_drot)
{
	const int idx = blockIdx.x * 256 + threadIdx.x;
	if (idx >= P) return;
	float s[GSR_SURF_ROW];
#pragma unroll
	for (int k = 0; k < GSR_SURF_ROW; k++) s[k] = 0.f;
	if (radii[idx] <= 0) {
		for (int k = 0; k < 3; k++) { dL_dmean2D[3 * (size_t)idx + k] = 0.f; dL_dcolor[3 * (size_t)idx + k] = 0.f; dL_dmean3D[3 * (size_t)idx + k] = 0.f; }
		dL_dopacity[idx] = 0.f;
		dL_dscale[2 * (size_t)idx] = 0.f; dL_dscale[2 * (size_t)idx + 1] = 0.f;
		*reinterpret_cast<float4*>(dL_drot + 4 * (size_t)idx) = make_float4(0.f, 0.f, 0.f, 0.f);
		return;
	}
	const uint32_t r0 = goff[idx], r1 = goff[idx + 1];
	for (uint32_t r = r0; r < r1; r++) {
		const float4* rp = reinterpret_cast<const float4*>(rows + (size_t)r * GSR_SURF_ROW);
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const float4 v = rp[i];
			s[4 * i] += v.x; s[4 * i + 1] += v.y; s[4 * i + 2] += v.z; s[4 * i + 3] += v.w;
		}
	}
	const SurfRec rec = recs[idx];
	const float* dM0 = s;       // dL/dTu = dL/dM[0][*]
	const float* dM1 = s + 3;   // dL/dTv
	const float* dM2 = s + 6;   // dL/dTw
	const float dMc[3][3] = {{dM0[0], dM1[0], dM2[0]}, {dM0[1], dM1[1], dM2[1]}, {dM0[2], dM1[2], dM2[2]}};   // [col][row]
	float Q[3][4];
	surf_q(cam->proj, W, H, Q);
	float inv_len;
	const float4 q = gs_act_rot(*reinterpret_cast<const float4*>(rotations + 4 * (size_t)idx), GSR_ACT_ROT_NORMALIZE, &inv_len);
	const M3 R = quat_to_R(q);
	const float su = scale_modifier * scales[2 * idx], sv = scale_modifier * scales[2 * idx + 1];
	// Q3^T applied to the three columns of dL/dM
	float dcol[3][3];
#pragma unroll
	for (int c = 0; c < 3; c++)
#pragma unroll
		for (int k = 0; k < 3; k++) dcol[c][k] = FMA(Q[2][k], dMc[c][2], FMA(Q[1][k], dMc[c][1], Q[0][k] * dMc[c][0]));
	float G[3][3];   // dL / d(column c of R)
	float dsu = 0.f, dsv = 0.f;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		dsu = FMA(R.m[0][k], dcol[0][k], dsu);
		dsv = FMA(R.m[1][k], dcol[1][k], dsv);
		G[0][k] = su * dcol[0][k];
		G[1][k] = sv * dcol[1][k];
	}
	// n_j = sgn sum_k view[4k + j] t_n[k]
	const float sgn = rec.q4.w;
	const float* view = cam->view;
	const float dn[3] = {s[13], s[14], s[15]};
#pragma unroll
	for (int k = 0; k < 3; k++) G[2][k] = sgn * FMA(view[4 * k + 2], dn[2], FMA(view[4 * k + 1], dn[1], view[4 * k] * dn[0]));
	// quat_to_R backward (r, x, y, z) = q
	const float r = q.x, x = q.y, y = q.z, z = q.w;
	float dq[4];
	dq[0] = 2.f * (-z * G[0][1] + y * G[0][2] + z * G[1][0] - x * G[1][2] - y * G[2][0] + x * G[2][1]);
	dq[1] = 2.f * (y * G[0][1] + z * G[0][2] + y * G[1][0] - 2.f * x * G[1][1] - r * G[1][2] + z * G[2][0] + r * G[2][1] - 2.f * x * G[2][2]);
	dq[2] = 2.f * (-2.f * y * G[0][0] + x * G[0][1] + r * G[0][2] + x * G[1][0] + z * G[1][2] - r * G[2][0] + z * G[2][1] - 2.f * y * G[2][2]);
	dq[3] = 2.f * (-2.f * z * G[0][0] - r * G[0][1] + x * G[0][2] + r * G[1][0] - 2.f * z * G[1][1] + y * G[1][2] + x * G[2][0] + y * G[2][1]);
	// through q / |q| (gs_act_rot)
	const float qg = q.x * dq[0] + q.y * dq[1] + q.z * dq[2] + q.w * dq[3];
	dq[0] = (dq[0] - q.x * qg) * inv_len; dq[1] = (dq[1] - q.y * qg) * inv_len;
	dq[2] = (dq[2] - q.z * qg) * inv_len; dq[3] = (dq[3] - q.w * qg) * inv_len;
	*reinterpret_cast<float4*>(dL_drot + 4 * (size_t)idx) = make_float4(dq[0], dq[1], dq[2], dq[3]);
	dL_dscale[2 * (size_t)idx] = scale_modifier * dsu;
	dL_dscale[2 * (size_t)idx + 1] = scale_modifier * dsv;
#pragma unroll
	for (int k = 0; k < 3; k++) dL_dmean3D[3 * (size_t)idx + k] = dcol[2][k];
	dL_dopacity[idx] = s[9];
#pragma unroll
	for (int c = 0; c < 3; c++) dL_dcolor[3 * (size_t)idx + c] = s[10 + c];
	const float M22 = rec.q2.x;
	dL_dmean2D[3 * (size_t)idx] = dM0[2] * M22 * (0.5f * (float)W);
	dL_dmean2D[3 * (size_t)idx + 1] = dM1[2] * M22 * (0.5f * (float)H);
	dL_dmean2D[3 * (size_t)idx + 2] = 0.f;
}

void launch_surfel_preprocess_bwd(int P, int W, int H, const float* means3D, const float* scales, float scale_modifier,
                                  const float* rotations, const int* radii, const GsCam* cam, const SurfRec* recs,
                                  const uint32_t* goff, const float* rows, float* dL_dmean2D, float* dL_dopacity, float* dL_dcolor,
                                  float* dL_dmean3D, float* dL_dscale, float* dL_drot, hipStream_t s)
{
	hipLaunchKernelGGL(surfel_preprocess_bwd_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, W, H, means3D, scales, scale_modifier,
	                   rotations, radii, cam, recs, goff, rows, dL_dmean2D, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dscale, dL_drot);
}

}  // namespace gsr
