// gsr_tsdf_rgbd.hip -- projective RGB-D fusion into a coloured block-sparse TSDF and coloured mesh extraction.
//
// Replaces, for the `tsdf` initializer (gaustudio/pipelines/initializers/mesh.py:445-514), the CPU library it calls:
//   o3d.pipelines.integration.ScalableTSDFVolume(voxel_length, sdf_trunc, color_type=RGB8).integrate(rgbd, K, E)   and
//   .extract_triangle_mesh()
// Open3D is not present here: the algorithm is restated from its published sources (ScalableTSDFVolume::Integrate,
// UniformTSDFVolume::IntegrateWithDepthToCameraDistanceMultiplier, ::ExtractTriangleMesh).  The authority for every
// operation and its order is the float32 model tests/tsdf_rgbd_model.py; PARITY UNPINNED against the library itself
// (DESIGN.md s15).  Unlike gsr_tsdf.hip (rays of a point cloud, VDBFusion) the integration is VOXEL-PROJECTIVE: every
// voxel of every block the frame's depth touches projects into the depth image and keeps a running average.
//
// MI355X design:
//   * the block hash and 64-bit keys of gsr_tsdf.hip (gsr_block_volume.h), a block's voxels AT its hash slot;
//   * voxels are SoA per block: five planes of 512 f32 -- tsdf, weight, r, g, b -- so a wave (one z-slice of 8 x 8
//     voxels, x fastest) reads and writes whole 256-byte lines, and its 64 voxel centres project to a compact footprint
//     of the depth image;
//   * touch (one thread per strided depth pixel) inserts the blocks of the pixel's +-sdf_trunc box and stamps their slots
//     with the frame number; integrate runs one workgroup per stamped slot.  One voxel is written by one thread in one
//     frame: float running averages, no atomics, deterministic;
//   * the matrices and intrinsics travel by value in the kernel argument block (scalar registers);
//   * extraction: the block marching cubes of gsr_block_volume.h with the float planes as its voxel format (PlaneVoxels): this
//     file has no marching-cubes kernel of its own.
// Plain float arithmetic, one rounding per operation (the library is compiled with -ffp-contract=off and correctly
// rounded divide / sqrt): the device results equal the model's bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsrast.h"
#include "gsr_block_volume.h"

namespace {

using gsr::pow2;
using gsr::tsdf_block_key;
using gsr::tsdf_decode_key;
using gsr::tsdf_find_or_insert;

constexpr int BLOCK_VOX = gsr::TSDF_BLOCK_VOX;
constexpr int PLANES = 5;                        // tsdf, weight, r, g, b
constexpr int BLOCK_F32 = PLANES * BLOCK_VOX;    // floats per hash slot (10 KiB)

struct Mat34 { float m[12]; };                   // rows 0..2 of a rigid 4x4, row-major
struct Pinhole { float fx, fy, cx, cy; };

// row r of M (x, y, z, 1), summed left to right
__device__ __forceinline__ float xform(const Mat34& M, int r, float x, float y, float z)
{
	return ((M.m[4 * r] * x + M.m[4 * r + 1] * y) + M.m[4 * r + 2] * z) + M.m[4 * r + 3];
}

// depth cleaning of the initializer (mesh.py:556-560), fused into the load: non-finite, negative and > depth_trunc -> 0
__device__ __forceinline__ float clean_depth(float d, float depth_trunc)
{
	return (d > 0.0f && d <= depth_trunc && d <= 3.4028235e38f) ? d : 0.0f;
}

// floor(v / block_size) as a block coordinate; false when it is not finite or outside the key's range
__device__ __forceinline__ bool block_coord(float v, float block_size, int& b)
{
	const float f = floorf(v / block_size);
	if (!(f >= -1048575.0f && f <= 1048575.0f)) return false;
	b = (int)f;
	return true;
}

// One thread per strided pixel: opens (and stamps) every block that intersects [p - sdf_trunc, p + sdf_trunc].
// Neighbouring pixels open the same blocks: a lane whose box of blocks equals that of the lane before it leaves the
// insertion to that lane (`filter`); counters (optional) [0] += insertions without the filter, [1] += insertions made.
__global__ __launch_bounds__(256) void ctsdf_touch_kernel(const float* __restrict__ depth, int W, int H, int stride, Pinhole K, Mat34 Einv,
                                                          float depth_trunc, float block_size, float sdf_trunc,
                                                          unsigned long long* __restrict__ keys, uint64_t mask, int* __restrict__ stamp,
                                                          int frame, uint32_t* __restrict__ status, int filter,
                                                          unsigned long long* __restrict__ counters)
{
	const int SW = (W + stride - 1) / stride, SH = (H + stride - 1) / stride;
	const int t = blockIdx.x * 256 + threadIdx.x;
	bool valid = t < SW * SH;
	int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
	if (valid) {
		const int u = (t % SW) * stride, v = (t / SW) * stride;
		const float d = clean_depth(depth[(size_t)v * W + u], depth_trunc);
		valid = d > 0.0f;
		if (valid) {
			const float x = (((float)u - K.cx) * d) / K.fx, y = (((float)v - K.cy) * d) / K.fy;
#pragma unroll
			for (int a = 0; a < 3; a++) {
				const float p = xform(Einv, a, x, y, d);
				valid = valid && block_coord(p - sdf_trunc, block_size, lo[a]) && block_coord(p + sdf_trunc, block_size, hi[a]);
			}
		}
	}
	// the lane before this one (all lanes take part in the shuffles)
	bool same = __shfl_up((int)valid, 1, 64) != 0 && (threadIdx.x & 63) != 0;
#pragma unroll
	for (int a = 0; a < 3; a++) {
		same = same && __shfl_up(lo[a], 1, 64) == lo[a];
		same = same && __shfl_up(hi[a], 1, 64) == hi[a];
	}
	if (!valid) return;
	const bool drop = filter && same;
	if (counters) {
		const unsigned long long n = (unsigned long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
		atomicAdd(&counters[0], n);
		if (!drop) atomicAdd(&counters[1], n);
	}
	if (drop) return;
	for (int bz = lo[2]; bz <= hi[2]; bz++)
		for (int by = lo[1]; by <= hi[1]; by++)
			for (int bx = lo[0]; bx <= hi[0]; bx++) {
				const int64_t slot = tsdf_find_or_insert(keys, mask, tsdf_block_key(bx, by, bz));
				if (slot < 0) { atomicOr(&status[0], 1u); return; }   // table full
				stamp[slot] = frame;                                  // same value from every lane: plain store
			}
}

// colour of pixel (u, v) in 0..255 units.  mode 0: u8 [H,W,3]; 1: f32 [H,W,3]; 2: f32 [3,H,W]; float input is quantised
// by the initializer's rule uint8(clip(x * 255, 0, 255)) with truncation (mesh.py:532-534; NaN -> 0)
__device__ __forceinline__ void load_rgb(const void* __restrict__ color, int mode, int W, int H, int u, int v, float* rgb)
{
	const size_t pix = (size_t)v * W + u;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		if (mode == 0) rgb[c] = (float)static_cast<const uint8_t*>(color)[3 * pix + c];
		else {
			const float x = static_cast<const float*>(color)[mode == 1 ? 3 * pix + c : (size_t)c * W * H + pix];
			rgb[c] = (float)(int)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f);
		}
	}
}

// One workgroup per touched block, one thread per voxel (x fastest: a wave = one z-slice of 8 x 8 voxels).
// UniformTSDFVolume::IntegrateWithDepthToCameraDistanceMultiplier with the multiplier evaluated per pixel.
__global__ __launch_bounds__(512) void ctsdf_integrate_kernel(const float* __restrict__ depth, const void* __restrict__ color, int color_mode,
                                                              int W, int H, Pinhole K, Mat34 E, float depth_trunc, float voxel_length,
                                                              float sdf_trunc, const unsigned long long* __restrict__ keys,
                                                              const int* __restrict__ touched, float* __restrict__ vox)
{
	const int slot = touched[blockIdx.x];
	int bx, by, bz;
	tsdf_decode_key(keys[slot], bx, by, bz);
	const int tid = threadIdx.x;
	const int i = bx * 8 + (tid & 7), j = by * 8 + ((tid >> 3) & 7), k = bz * 8 + (tid >> 6);
	const float X = ((float)i + 0.5f) * voxel_length, Y = ((float)j + 0.5f) * voxel_length, Z = ((float)k + 0.5f) * voxel_length;
	const float cz = xform(E, 2, X, Y, Z);
	if (!(cz > 0.0f)) return;                                       // behind the camera
	const float cxx = xform(E, 0, X, Y, Z), cyy = xform(E, 1, X, Y, Z);
	const float uf = ((cxx * K.fx) / cz + K.cx) + 0.5f, vf = ((cyy * K.fy) / cz + K.cy) + 0.5f;
	if (!(uf >= 0.0001f && uf < (float)W - 0.0001f && vf >= 0.0001f && vf < (float)H - 0.0001f)) return;
	const int u = (int)uf, v = (int)vf;                             // in [0, W) x [0, H) by the test above
	const float d = clean_depth(depth[(size_t)v * W + u], depth_trunc);
	if (!(d > 0.0f)) return;
	const float a = ((float)u - K.cx) / K.fx, b = ((float)v - K.cy) / K.fy;
	const float mult = sqrtf((a * a + b * b) + 1.0f);
	const float sdf = (d - cz) * mult;
	if (!(sdf > -sdf_trunc)) return;
	const float tv = fminf(1.0f, sdf / sdf_trunc);
	float rgb[3];
	load_rgb(color, color_mode, W, H, u, v, rgb);
	float* cell = vox + (size_t)slot * BLOCK_F32 + tid;
	const float w = cell[BLOCK_VOX], w1 = w + 1.0f;
	cell[0] = (cell[0] * w + tv) / w1;
	cell[BLOCK_VOX] = w1;
#pragma unroll
	for (int c = 0; c < 3; c++) cell[(2 + c) * BLOCK_VOX] = (cell[(2 + c) * BLOCK_VOX] * w + rgb[c]) / w1;
}

// dump of the listed blocks for tests: tsdf, weight [n,512] and colour [n,512,3]
__global__ __launch_bounds__(512) void ctsdf_export_kernel(const float* __restrict__ vox, const uint32_t* __restrict__ slots,
                                                           float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color)
{
	const float* cell = vox + (size_t)slots[blockIdx.x] * BLOCK_F32 + threadIdx.x;
	const size_t dst = (size_t)blockIdx.x * BLOCK_VOX + threadIdx.x;
	tsdf[dst] = cell[0];
	weight[dst] = cell[BLOCK_VOX];
	for (int c = 0; c < 3; c++) color[3 * dst + c] = cell[(2 + c) * BLOCK_VOX];
}

// ---- marching cubes over the occupied blocks: the float planes as a voxel format of the scheme of gsr_block_volume.h ----
// A cube is meshed iff all 8 corners have weight > 0 and weight >= min_weight.  A vertex's colour is c0 + r (c1 - c0) between
// the two voxels of its edge, kept inside [min, max] of the two, / 255.
struct PlaneVoxels {
	static constexpr int SLOT_ELEMS = BLOCK_F32;
	static constexpr bool COLORS = true;
	const float* vox;
	float voxel, min_weight;
	__device__ bool corner(size_t at, float& f) const
	{
		const float w = vox[at + BLOCK_VOX];
		f = vox[at];
		return w > 0.0f && !(w < min_weight);
	}
	__device__ float centre(int idx) const { return ((float)idx + 0.5f) * voxel; }
	__device__ float colour(size_t at0, size_t at1, int c, float r) const
	{
		const float q0 = vox[at0 + (2 + c) * BLOCK_VOX], q1 = vox[at1 + (2 + c) * BLOCK_VOX];
		return fminf(fmaxf(q0 + r * (q1 - q0), fminf(q0, q1)), fmaxf(q0, q1)) / 255.0f;
	}
};

bool rigid_ok(const float* m)
{
	if (!m) return false;
	for (int i = 0; i < 12; i++)
		if (!(m[i] == m[i]) || m[i] > 3.0e38f || m[i] < -3.0e38f) return false;
	return true;
}

}  // namespace

extern "C" {

int gsr_ctsdf_touch(const float* depth, int width, int height, int stride, const float intrinsic[4], const float cam_to_world[12],
                    float depth_trunc, float voxel_length, float sdf_trunc, uint64_t* block_keys, uint64_t capacity,
                    int* slot_stamp, int frame, uint32_t* status, int lane_filter, uint64_t* counters, void* stream)
{
	if (!depth || !intrinsic || !rigid_ok(cam_to_world) || !block_keys || !slot_stamp || !status || !pow2(capacity) || width <= 0 ||
	    height <= 0 || stride <= 0 || !(voxel_length > 0.f) || !(sdf_trunc > 0.f) || frame <= 0)
		return GSR_ERR_ARG;
	if (!(intrinsic[0] != 0.f) || !(intrinsic[1] != 0.f)) return GSR_ERR_ARG;
	const long long n = (long long)((width + stride - 1) / stride) * ((height + stride - 1) / stride);
	if (n >= (1ll << 31) - 256) return GSR_ERR_ARG;
	Pinhole K = {intrinsic[0], intrinsic[1], intrinsic[2], intrinsic[3]};
	Mat34 M;
	for (int i = 0; i < 12; i++) M.m[i] = cam_to_world[i];
	hipLaunchKernelGGL(ctsdf_touch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth, width, height, stride,
	                   K, M, depth_trunc, 8.0f * voxel_length, sdf_trunc, reinterpret_cast<unsigned long long*>(block_keys), capacity - 1,
	                   slot_stamp, frame, status, lane_filter, reinterpret_cast<unsigned long long*>(counters));
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_ctsdf_integrate(const float* depth, const void* color, int color_mode, int width, int height, const float intrinsic[4],
                        const float world_to_cam[12], float depth_trunc, float voxel_length, float sdf_trunc,
                        const uint64_t* block_keys, const int* touched_slots, int num_touched, float* voxels, void* stream)
{
	if (num_touched <= 0) return GSR_OK;
	if (!depth || !color || color_mode < 0 || color_mode > 2 || !intrinsic || !rigid_ok(world_to_cam) || !block_keys || !touched_slots ||
	    !voxels || width <= 0 || height <= 0 || !(voxel_length > 0.f) || !(sdf_trunc > 0.f))
		return GSR_ERR_ARG;
	Pinhole K = {intrinsic[0], intrinsic[1], intrinsic[2], intrinsic[3]};
	Mat34 M;
	for (int i = 0; i < 12; i++) M.m[i] = world_to_cam[i];
	hipLaunchKernelGGL(ctsdf_integrate_kernel, dim3(num_touched), dim3(512), 0, (hipStream_t)stream, depth, color, color_mode, width, height,
	                   K, M, depth_trunc, voxel_length, sdf_trunc, reinterpret_cast<const unsigned long long*>(block_keys), touched_slots,
	                   voxels);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_ctsdf_export_blocks(const float* voxels, const uint32_t* block_slots, int num_blocks, float* tsdf, float* weight, float* color,
                            void* stream)
{
	if (num_blocks <= 0) return GSR_OK;
	if (!voxels || !block_slots || !tsdf || !weight || !color) return GSR_ERR_ARG;
	hipLaunchKernelGGL(ctsdf_export_kernel, dim3(num_blocks), dim3(512), 0, (hipStream_t)stream, voxels, block_slots, tsdf, weight, color);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_ctsdf_mc_classify(const uint64_t* block_keys, uint64_t capacity, const float* voxels, const uint32_t* block_slots, int num_blocks,
                          const uint32_t* slot_to_block, float min_weight, uint8_t* cases, uint32_t* edge_flags,
                          uint32_t* block_num_vertices, uint32_t* block_num_triangles, void* stream)
{
	if (num_blocks <= 0) return GSR_OK;
	if (!block_keys || !voxels || !block_slots || !slot_to_block || !cases || !edge_flags || !block_num_vertices || !block_num_triangles ||
	    !pow2(capacity))
		return GSR_ERR_ARG;
	const PlaneVoxels vol = {voxels, 0.0f, min_weight};
	return gsr::launch_block_mc_classify(vol, block_keys, capacity, block_slots, num_blocks, slot_to_block, cases, edge_flags,
	                                     block_num_vertices, block_num_triangles, (hipStream_t)stream);
}

int gsr_ctsdf_mc_emit(const uint64_t* block_keys, uint64_t capacity, const float* voxels, const uint32_t* block_slots, int num_blocks,
                      const uint32_t* slot_to_block, float voxel_length, const uint8_t* cases, const uint32_t* edge_flags,
                      const uint32_t* block_vertex_offset, const uint32_t* block_triangle_offset, uint32_t* vertex_base, float* vertices,
                      float* colors, int* triangles, void* stream)
{
	if (num_blocks <= 0) return GSR_OK;
	if (!block_keys || !voxels || !block_slots || !slot_to_block || !cases || !edge_flags || !block_vertex_offset || !block_triangle_offset ||
	    !vertex_base || !vertices || !colors || !triangles || !pow2(capacity))
		return GSR_ERR_ARG;
	const PlaneVoxels vol = {voxels, voxel_length, 0.0f};
	return gsr::launch_block_mc_emit(vol, block_keys, capacity, block_slots, num_blocks, slot_to_block, cases, edge_flags, block_vertex_offset,
	                                 block_triangle_offset, vertex_base, vertices, colors, triangles, (hipStream_t)stream);
}

}  // extern "C"
