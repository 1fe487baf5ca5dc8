// gsr_block_volume.h -- what the block-sparse volumes (gsr_tsdf.hip: packed 64-bit voxels; gsr_tsdf_rgbd.hip: five float planes
// per block) share on the device: the block hash, and the marching cubes over the occupied blocks.
//
// Marching cubes is one scheme for every voxel format: classify (cube case per voxel, edge flags OR-ed into the edges'
// owners) -> count (per block totals for the host's scan) -> vertices -> triangles, with shared vertices (a voxel owns the
// three edges that leave its minimum corner) and no atomics in the emit passes.  One workgroup per occupied block, one
// thread per voxel; blocks[] lists hash slots in a caller-chosen, deterministic order, cases / flags / vbase are indexed by
// that COMPACT block index and cidx maps hash slot -> compact index.  Only the classify and vertices passes read voxels:
// they are templates over a by-value policy struct V that answers what differs between formats and nothing else --
//   V::SLOT_ELEMS                 elements of V's storage per hash slot (a voxel's first element is at slot * SLOT_ELEMS + local)
//   bool V::corner(at, f)         f = tsdf of the voxel at element `at`; returns whether it may be a corner of an extracted cube
//   float V::centre(idx)          world coordinate of the centre of voxel index idx along one axis (the format's own float expression:
//                                 each equals its model's bit for bit)
//   V::COLORS, V::colour(at0, at1, c, r)   whether vertices carry colours, and channel c between two voxels at ratio r
//   V::voxel                      edge length of a voxel
// The count and triangles passes read cases / flags / vbase only: launch_tsdf_mc_count, launch_tsdf_mc_triangles (gsr_tsdf.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsrast.h"
#include "gsr_mc_tables.h"

namespace gsr {

// --- block hash: 8^3-voxel blocks, 64-bit keys of three 21-bit biased block coordinates, open addressing with linear
// probing; a block's voxels live at its hash slot ---
constexpr uint64_t TSDF_EMPTY = ~0ull;
constexpr int TSDF_BLOCK_VOX = 512;

inline bool pow2(uint64_t v) { return v && !(v & (v - 1)); }   // hash capacities

__host__ __device__ __forceinline__ uint64_t tsdf_block_key(int bx, int by, int bz)
{
	const uint64_t B = 1u << 20;   // block coordinates in (-2^20, 2^20)
	return ((uint64_t)(bx + (int)B) << 42) | ((uint64_t)(by + (int)B) << 21) | (uint64_t)(bz + (int)B);
}
__host__ __device__ __forceinline__ void tsdf_decode_key(uint64_t key, int& bx, int& by, int& bz)
{
	const int B = 1 << 20;
	bx = (int)((key >> 42) & 0x1fffff) - B;
	by = (int)((key >> 21) & 0x1fffff) - B;
	bz = (int)(key & 0x1fffff) - B;
}
__device__ __forceinline__ uint64_t tsdf_mix64(uint64_t x)
{
	x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
	x ^= x >> 27; x *= 0x94d049bb133111ebull;
	x ^= x >> 31;
	return x;
}
// returns the slot of `key`, inserting it if absent; -1 when the table is full (probe limit)
__device__ inline int64_t tsdf_find_or_insert(unsigned long long* keys, uint64_t mask, uint64_t key)
{
	uint64_t slot = tsdf_mix64(key) & mask;
	for (uint64_t probe = 0; probe <= mask; probe++) {
		unsigned long long k = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);
		if (k == key) return (int64_t)slot;
		if (k == TSDF_EMPTY) {
			const unsigned long long old = atomicCAS(&keys[slot], (unsigned long long)TSDF_EMPTY, (unsigned long long)key);
			if (old == TSDF_EMPTY || old == key) return (int64_t)slot;
		}
		slot = (slot + 1) & mask;
	}
	return -1;
}
__device__ inline int64_t tsdf_find_slot(const unsigned long long* keys, uint64_t mask, uint64_t key)
{
	uint64_t slot = tsdf_mix64(key) & mask;
	for (uint64_t probe = 0; probe <= mask; probe++) {
		const unsigned long long k = keys[slot];
		if (k == key) return (int64_t)slot;
		if (k == TSDF_EMPTY) return -1;
		slot = (slot + 1) & mask;
	}
	return -1;
}

// --- marching cubes over the occupied blocks ---
// The two voxel-format-independent passes (gsr_tsdf.hip): per-block vertex / triangle totals from cases[] and flags[], and
// the triangles through the edge owners' vbase[].  Return GSR_OK or GSR_ERR_HIP.
int launch_tsdf_mc_count(int num_blocks, const uint8_t* cases, const uint32_t* flags, uint32_t* block_nv, uint32_t* block_nt, hipStream_t s);
int launch_tsdf_mc_triangles(const uint64_t* keys, uint64_t capacity, const uint32_t* blocks, int num_blocks, const uint32_t* cidx,
                             const uint8_t* cases, const uint32_t* flags, const uint32_t* vbase, const uint32_t* block_toff,
                             int* triangles, hipStream_t s);

// s_nb[8] = hash slots of the 2x2x2 blocks starting at the workgroup's block `slot` (-1 = absent), index dz*4+dy*2+dx: a cube
// of the block's last layer of voxels has corners in them.  s_b (optional) = the block's coordinates.  Ends with a barrier.
__device__ __forceinline__ void neighbour_slots(const unsigned long long* __restrict__ keys, uint64_t mask, uint32_t slot, int64_t* s_nb,
                                                int* s_b)
{
	if (threadIdx.x < 8) {
		int bx, by, bz;
		tsdf_decode_key(keys[slot], bx, by, bz);
		if (threadIdx.x == 0 && s_b) { s_b[0] = bx; s_b[1] = by; s_b[2] = bz; }
		s_nb[threadIdx.x] = threadIdx.x == 0 ? (int64_t)slot
		                                     : tsdf_find_slot(keys, mask, tsdf_block_key(bx + (threadIdx.x & 1), by + ((threadIdx.x >> 1) & 1), bz + (threadIdx.x >> 2)));
	}
	__syncthreads();
}

// the voxel at local coordinates (lx,ly,lz) in [0,8] of the 2x2x2 block neighbourhood, as an element index into voxel storage
// with `slot_elems` elements per hash slot; -1 = block absent
__device__ __forceinline__ int64_t voxel_at(const int64_t* nb, int slot_elems, int lx, int ly, int lz)
{
	const int64_t s = nb[((lz >> 3) << 2) | ((ly >> 3) << 1) | (lx >> 3)];
	return s < 0 ? -1 : s * slot_elems + (((lz & 7) << 6) | ((ly & 7) << 3) | (lx & 7));
}

// exclusive scan of a per-voxel count inside a 512-thread block; returns this thread's offset.  The barrier at the end lets
// the caller use s_w (8 words) again.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_w)
{
	uint32_t incl = v;
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
		if (lane >= o) incl += t;
	}
	if (lane == 63) s_w[wv] = incl;
	__syncthreads();
	uint32_t base = 0;
	for (int w = 0; w < wv; w++) base += s_w[w];
	__syncthreads();
	return base + incl - v;
}

// classify: per voxel the case (u8) of the cube whose minimum corner it is -- 0 when the cube is not extractable -- and,
// OR-ed into the owning voxels, which of their three edges carry a vertex.  A corner is inside iff its tsdf < 0.
template <class V>
__global__ __launch_bounds__(512) void block_mc_classify_kernel(V vol, const unsigned long long* __restrict__ keys, uint64_t mask,
                                                                const uint32_t* __restrict__ blocks, const uint32_t* __restrict__ cidx,
                                                                uint8_t* __restrict__ cases, uint32_t* __restrict__ flags)
{
	__shared__ int64_t s_nb[8];
	neighbour_slots(keys, mask, blocks[blockIdx.x], s_nb, nullptr);
	const int lx = threadIdx.x & 7, ly = (threadIdx.x >> 3) & 7, lz = threadIdx.x >> 6;
	int cs = 0;
	bool ok = true;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		// a corner in a block that was never allocated makes the cube non-extractable (its edge owners have no storage)
		const int64_t at = voxel_at(s_nb, V::SLOT_ELEMS, lx + gsr_mc_corner[i][0], ly + gsr_mc_corner[i][1], lz + gsr_mc_corner[i][2]);
		float f;
		if (at < 0 || !vol.corner((size_t)at, f)) { ok = false; break; }
		if (f < 0.0f) cs |= 1 << i;
	}
	if (!ok || cs == 255) cs = 0;
	cases[(size_t)blockIdx.x * TSDF_BLOCK_VOX + threadIdx.x] = (uint8_t)cs;
	if (cs == 0) return;
	const uint32_t em = gsr_mc_edge_mask[cs];
	for (int e = 0; e < 12; e++) {
		if (!((em >> e) & 1)) continue;
		const int o = gsr_mc_edge_owner[e];
		const int ox = lx + gsr_mc_corner[o][0], oy = ly + gsr_mc_corner[o][1], oz = lz + gsr_mc_corner[o][2];
		const int64_t s = s_nb[((oz >> 3) << 2) | ((oy >> 3) << 1) | (ox >> 3)];   // present: the cube was extractable
		atomicOr(&flags[(size_t)cidx[s] * TSDF_BLOCK_VOX + (((oz & 7) << 6) | ((oy & 7) << 3) | (ox & 7))], 1u << gsr_mc_edge_axis[e]);
	}
}

// vertices (and their colours): vbase[voxel] = index of the voxel's first vertex.  A vertex lies at the linear zero crossing
// between the two voxel centres of its edge, a0 * voxel / (a0 + a1) from the owner's, a = |tsdf|.
template <class V>
__global__ __launch_bounds__(512) void block_mc_vertices_kernel(V vol, const unsigned long long* __restrict__ keys, uint64_t mask,
                                                                const uint32_t* __restrict__ blocks, const uint32_t* __restrict__ flags,
                                                                const uint32_t* __restrict__ block_voff, uint32_t* __restrict__ vbase,
                                                                float* __restrict__ vertices, float* __restrict__ colors)
{
	__shared__ int64_t s_nb[8];
	__shared__ uint32_t s_w[8];
	__shared__ int s_b[3];
	neighbour_slots(keys, mask, blocks[blockIdx.x], s_nb, s_b);
	const size_t i = (size_t)blockIdx.x * TSDF_BLOCK_VOX + threadIdx.x;
	const uint32_t fl = flags[i] & 7u;
	const uint32_t off = block_voff[blockIdx.x] + block_excl_scan(__popc(fl), s_w);
	vbase[i] = off;
	if (!fl) return;
	const int lx = threadIdx.x & 7, ly = (threadIdx.x >> 3) & 7, lz = threadIdx.x >> 6;
	const size_t at0 = (size_t)voxel_at(s_nb, V::SLOT_ELEMS, lx, ly, lz);
	float f0;
	vol.corner(at0, f0);
	const float base[3] = {vol.centre(s_b[0] * 8 + lx), vol.centre(s_b[1] * 8 + ly), vol.centre(s_b[2] * 8 + lz)};
	uint32_t k = off;
	for (int a = 0; a < 3; a++) {
		if (!((fl >> a) & 1)) continue;
		const size_t kv = 3 * (size_t)k++;
		const int64_t at1 = voxel_at(s_nb, V::SLOT_ELEMS, lx + (a == 0), ly + (a == 1), lz + (a == 2));
		if (at1 < 0) continue;   // never with flags the classify pass wrote (an extractable cube flagged the edge); they are the caller's
		float f1;
		vol.corner((size_t)at1, f1);
		const float a0 = fabsf(f0), a1 = fabsf(f1);
		float p[3] = {base[0], base[1], base[2]};
		p[a] += a0 * vol.voxel / (a0 + a1);
		const float r = a0 / (a0 + a1);
#pragma unroll
		for (int c = 0; c < 3; c++) {
			vertices[kv + c] = p[c];
			if constexpr (V::COLORS) colors[kv + c] = vol.colour(at0, (size_t)at1, c, r);
		}
	}
}

// host side of the two voxel-reading passes; the callers have checked their arguments
template <class V>
int launch_block_mc_classify(const V& vol, const uint64_t* keys, uint64_t capacity, const uint32_t* blocks, int num_blocks, const uint32_t* cidx,
                             uint8_t* cases, uint32_t* flags, uint32_t* block_nv, uint32_t* block_nt, hipStream_t s)
{
	if (hipMemsetAsync(flags, 0, sizeof(uint32_t) * (size_t)num_blocks * TSDF_BLOCK_VOX, s) != hipSuccess) return GSR_ERR_HIP;
	hipLaunchKernelGGL(block_mc_classify_kernel<V>, dim3(num_blocks), dim3(512), 0, s, vol, reinterpret_cast<const unsigned long long*>(keys),
	                   capacity - 1, blocks, cidx, cases, flags);
	if (hipGetLastError() != hipSuccess) return GSR_ERR_HIP;
	return launch_tsdf_mc_count(num_blocks, cases, flags, block_nv, block_nt, s);
}

template <class V>
int launch_block_mc_emit(const V& vol, const uint64_t* keys, uint64_t capacity, const uint32_t* blocks, int num_blocks, const uint32_t* cidx,
                         const uint8_t* cases, const uint32_t* flags, const uint32_t* block_voff, const uint32_t* block_toff,
                         uint32_t* vbase, float* vertices, float* colors, int* triangles, hipStream_t s)
{
	hipLaunchKernelGGL(block_mc_vertices_kernel<V>, dim3(num_blocks), dim3(512), 0, s, vol, reinterpret_cast<const unsigned long long*>(keys),
	                   capacity - 1, blocks, flags, block_voff, vbase, vertices, colors);
	if (hipGetLastError() != hipSuccess) return GSR_ERR_HIP;
	return launch_tsdf_mc_triangles(keys, capacity, blocks, num_blocks, cidx, cases, flags, vbase, block_toff, triangles, s);
}

}  // namespace gsr
