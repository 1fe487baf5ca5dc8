// gsr_hull.hip -- visual hull: silhouette masks packed to one bit per pixel, and the carve of a voxel grid against them.
//
// Replaces, for the `VisualHull` initializer (gaustudio/pipelines/initializers/mask.py:38-71), its per-camera torch program:
//   inside_view = camera.insideView(points_world); inside_mask = camera.insideView(points_world[idx], camera.mask); filled &= ...
// (Camera.insideView, gaustudio/datasets/__init__.py:268-305) -- about ten elementwise passes per camera over a materialised
// [R^3, 3] point array.  Here a voxel is a thread, its three coordinates come from per-axis tables (the reference's grid is
// separable), and the cameras are a loop over registers: per camera 16 matrix floats + 5 integers arrive through scalar loads
// (the table index is wave-uniform), one mask word through a vector load.  The authority for every operation and its order
// is the float32 model tests/visual_hull_model.py; the results equal it bit for bit (no contraction, correctly rounded divide).
//
// MI355X design:
//   * one thread per voxel, the LAST grid axis fastest across the lanes of a wave: neighbouring lanes project to neighbouring
//     pixels, so a wave's 64 mask reads fall into a few 32-bit words of one or two mask rows, and the u8 output is written in
//     whole 64-byte runs;
//   * a lane stops at its first carving camera; the wave leaves the camera loop when __ballot(alive) == 0.  A grid is mostly
//     empty space that the first few silhouettes carve, so most waves run a handful of the cameras;
//   * masks are bits (an 800 x 800 view: 80 KB instead of 640 KB as u8 / 2.5 MB as float): 100 views stay in the L2;
//   * the filled count is one integer atomicAdd per wave (the sum of integers: deterministic).  No float atomics, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsrast.h"

namespace {

static_assert(sizeof(gsr_hull_camera) == 96, "gsr_hull_camera is 24 words");

// One wave per 64 consecutive pixels of one mask row: the ballot of "pixel is set" is two words of the packed row.
// MODE 0: one byte per pixel (uint8 / bool), 1: float32.  A pixel is set iff its value is nonzero (what .bool() does: NaN is set).
template <int MODE>
__global__ __launch_bounds__(256) void hull_pack_kernel(const void* __restrict__ mask, int W, int H, int segs, uint32_t* __restrict__ words,
                                                        int row_stride)
{
	const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6;
	const int lane = threadIdx.x & 63;
	const uint32_t row = wave / (uint32_t)segs, seg = wave % (uint32_t)segs;
	if (row >= (uint32_t)H) return;                                  // whole waves only: `row` is wave-uniform
	const int col = (int)seg * 64 + lane;
	bool set = false;
	if (col < W) {
		const size_t p = (size_t)row * W + col;
		if (MODE == 0) set = static_cast<const uint8_t*>(mask)[p] != 0;
		else set = static_cast<const float*>(mask)[p] != 0.0f;
	}
	const unsigned long long b = __ballot(set);
	const int w = (int)seg * 2 + lane;                               // lanes 0 and 1 store the two words
	if (lane < 2 && w * 32 < W) words[(size_t)row * row_stride + w] = (uint32_t)(b >> (32 * lane));
}

// ((x m[c] + y m[4+c]) + z m[8+c]) + m[12+c]: column c of [x,y,z,1] @ M, the order of the model
__device__ __forceinline__ float clip_col(const float* m, int c, float x, float y, float z)
{
	return ((x * m[c] + y * m[4 + c]) + z * m[8 + c]) + m[12 + c];
}

// Flat voxel t = (i r1 + j) r2 + k sits at (ax_x[j], ax_y[i], ax_z[k]): np.meshgrid's default 'xy' indexing (mask.py:43-48).
__global__ __launch_bounds__(256) void hull_carve_kernel(const float* __restrict__ ax_x, const float* __restrict__ ax_y,
                                                         const float* __restrict__ ax_z, uint32_t r1, uint32_t r2, uint32_t n,
                                                         const gsr_hull_camera* __restrict__ cams, int num_cameras,
                                                         const uint32_t* __restrict__ words, uint8_t* __restrict__ filled,
                                                         unsigned int* __restrict__ count, int* __restrict__ carved_by)
{
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	const bool valid = t < n;
	bool alive = valid;
	int who = -1;
	float x = 0.0f, y = 0.0f, z = 0.0f;
	if (valid) {
		const uint32_t ij = t / r2, k = t - ij * r2, i = ij / r1, j = ij - i * r1;
		x = ax_x[j]; y = ax_y[i]; z = ax_z[k];
	}
	for (int c = 0; c < num_cameras; c++) {
		if (__ballot(alive) == 0) break;                             // wave-uniform: every voxel of the wave is carved
		const gsr_hull_camera cam = cams[c];                         // wave-uniform address: scalar loads
		if (!alive) continue;
		// Camera.insideView (datasets/__init__.py:277-303)
		const float cx = clip_col(cam.m, 0, x, y, z), cy = clip_col(cam.m, 1, x, y, z);
		const float cz = clip_col(cam.m, 2, x, y, z), cw = clip_col(cam.m, 3, x, y, z);
		const float nx = cx / cw, ny = cy / cw;
		bool keep = cz > 0.0f && nx >= -1.0f && nx <= 1.0f && ny >= -1.0f && ny <= 1.0f;   // false for NaN
		if (keep && cam.has_mask) {
			const float fx = ((nx + 1.0f) * 0.5f) * (float)cam.width, fy = ((1.0f + ny) * 0.5f) * (float)cam.height;
			int px = (int)fx, py = (int)fy;                          // in [0, W] x [0, H]: truncation, then the clamp
			px = min(max(px, 0), cam.width - 1);
			py = min(max(py, 0), cam.height - 1);
			const uint32_t w = words[(size_t)cam.word_offset + (size_t)py * cam.row_stride + (px >> 5)];
			keep = (w >> (px & 31)) & 1u;
		}
		if (!keep) { alive = false; who = c; }
	}
	if (valid) {
		filled[t] = alive ? 1 : 0;
		if (carved_by) carved_by[t] = who;
	}
	const unsigned long long b = __ballot(alive);
	if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned int)__popcll(b));
}

}  // namespace

extern "C" {

int gsr_hull_pack_masks(const void* mask, int dtype, int width, int height, uint32_t* mask_words, uint64_t word_offset, int row_stride,
                        uint64_t num_words, void* stream)
{
	if (!mask || !mask_words || dtype < 0 || dtype > 1 || width <= 0 || height <= 0 || width > (1 << 20) || height > (1 << 20))
		return GSR_ERR_ARG;
	if (row_stride < (width + 31) / 32 || word_offset > num_words || (uint64_t)height * (uint64_t)row_stride > num_words - word_offset)
		return GSR_ERR_ARG;
	const int segs = (width + 63) / 64;
	const long long waves = (long long)segs * height;
	if (waves >= (1ll << 32) - 4) return GSR_ERR_ARG;
	const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
	if (dtype == 0)
		hipLaunchKernelGGL(hull_pack_kernel<0>, grid, block, 0, (hipStream_t)stream, mask, width, height, segs, mask_words + word_offset,
		                   row_stride);
	else
		hipLaunchKernelGGL(hull_pack_kernel<1>, grid, block, 0, (hipStream_t)stream, mask, width, height, segs, mask_words + word_offset,
		                   row_stride);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_hull_carve(const float* axis_x, const float* axis_y, const float* axis_z, int r0, int r1, int r2,
                   const gsr_hull_camera* cameras_host, gsr_hull_camera* cameras_device, int num_cameras, const uint32_t* mask_words,
                   uint64_t num_words, uint8_t* filled, uint32_t* count, int* carved_by, void* stream)
{
	if (!axis_x || !axis_y || !axis_z || !cameras_host || !cameras_device || !filled || !count || num_cameras <= 0 || r0 <= 0 || r1 <= 0 ||
	    r2 <= 0)
		return GSR_ERR_ARG;
	const unsigned long long n = (unsigned long long)r0 * (unsigned long long)r1 * (unsigned long long)r2;
	if (n >= (1ull << 31)) return GSR_ERR_ARG;
	// every mask read of the kernel stays inside [word_offset, word_offset + height * row_stride) of its camera: checked here
	for (int c = 0; c < num_cameras; c++) {
		const gsr_hull_camera& C = cameras_host[c];
		if (C.width <= 0 || C.height <= 0 || C.width > (1 << 20) || C.height > (1 << 20)) return GSR_ERR_ARG;
		if (!C.has_mask) continue;
		if (!mask_words || C.row_stride < (C.width + 31) / 32 || C.word_offset > num_words ||
		    (uint64_t)C.height * (uint64_t)C.row_stride > num_words - C.word_offset)
			return GSR_ERR_ARG;
	}
	hipStream_t s = (hipStream_t)stream;
	if (hipMemcpyAsync(cameras_device, cameras_host, sizeof(gsr_hull_camera) * (size_t)num_cameras, hipMemcpyHostToDevice, s) != hipSuccess)
		return GSR_ERR_HIP;
	if (hipMemsetAsync(count, 0, sizeof(uint32_t), s) != hipSuccess) return GSR_ERR_HIP;
	hipLaunchKernelGGL(hull_carve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, axis_x, axis_y, axis_z, (uint32_t)r1,
	                   (uint32_t)r2, (uint32_t)n, cameras_device, num_cameras, mask_words, filled, count, carved_by);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
