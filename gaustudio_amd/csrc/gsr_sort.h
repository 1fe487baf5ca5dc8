// gsr_sort.h -- the device exclusive scan and the stable LSD radix sort (kernels, buffers and the pass loop) shared by
// gsr_knn.hip (fusion records grouped by Gaussian id), gsr_mesh.hip (faces binned by tile, vertex corners grouped by vertex),
// gsr_mesh_clean.hip (edges grouped by vertex pair, triangles by cluster), gsr_voxel.hip (triangle-voxel pairs by voxel) and
// gsr_psr.hip (points by grid cell); the scan alone serves more stages of the same files.  Everything here has internal
// linkage: each file that includes it gets its own kernels (no relocatable device code in this library).
#ifndef GSR_SORT_H_INCLUDED
#define GSR_SORT_H_INCLUDED
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/gsrast.h"
#include "gsr_ws.h"

namespace {

// ------------------------------------------------------------------------------------------------------ scans
// exclusive scan of n values in three passes over 1024-element tiles; `part` holds ceil(n/1024) + 1 values; total in out[n]
template <class T>
__global__ void __launch_bounds__(256) scan_sums(const T* __restrict__ in, int n, T* __restrict__ part)
{
	__shared__ T red[256];
	const int base = blockIdx.x * 1024;
	T s = 0;
	for (int j = 0; j < 4; j++) {
		const int i = base + j * 256 + threadIdx.x;
		if (i < n) s += in[i];
	}
	red[threadIdx.x] = s;
	__syncthreads();
	for (int w = 128; w > 0; w >>= 1) {
		if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
		__syncthreads();
	}
	if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
template <class T>
__device__ __forceinline__ T block_incl_scan(T* buf, T v)
{
	buf[threadIdx.x] = v;
	__syncthreads();
	for (int o = 1; o < 1024; o <<= 1) {
		const T y = (int)threadIdx.x >= o ? buf[threadIdx.x - o] : 0;
		__syncthreads();
		buf[threadIdx.x] += y;
		__syncthreads();
	}
	return buf[threadIdx.x];
}
template <class T>
__global__ void __launch_bounds__(1024) scan_parts(T* part, int np)
{
	__shared__ T buf[1024];
	T carry = 0;
	for (int b = 0; b < np; b += 1024) {
		const int i = b + threadIdx.x;
		const T v = i < np ? part[i] : 0;
		const T incl = block_incl_scan(buf, v);
		if (i < np) part[i] = carry + incl - v;
		const T tot = buf[1023];
		__syncthreads();
		carry += tot;
	}
	if (threadIdx.x == 0) part[np] = carry;
}
template <class T>
__global__ void __launch_bounds__(1024) scan_apply(const T* __restrict__ in, int n, const T* __restrict__ part, int np, T* __restrict__ out)
{
	__shared__ T buf[1024];
	const int i = blockIdx.x * 1024 + threadIdx.x;
	const T v = i < n ? in[i] : 0;
	const T incl = block_incl_scan(buf, v);
	if (i < n) out[i] = part[blockIdx.x] + incl - v;
	if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = part[np];
}
int scan_part_len(long long n) { return (int)(n / 1024 + 2); }   // elements of `part` for a scan of n values
// out[n + 1]: exclusive scan and total
template <class T>
int exclusive_scan(const T* in, int n, T* out, T* part, hipStream_t s)
{
	const int np = (n + 1023) / 1024;
	if (np == 0) return hipMemsetAsync(out, 0, sizeof(T), s) == hipSuccess ? GSR_OK : GSR_ERR_HIP;
	hipLaunchKernelGGL(scan_sums<T>, dim3(np), dim3(256), 0, s, in, n, part);
	hipLaunchKernelGGL(scan_parts<T>, dim3(1), dim3(1024), 0, s, part, np);
	hipLaunchKernelGGL(scan_apply<T>, dim3(np), dim3(1024), 0, s, in, n, part, np, out);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

// ------------------------------------------------------------------------------------------------------ stable radix sort
// One 8-bit counting-sort pass over (keys, vals): radix_hist, an exclusive scan of the digit-major histogram, radix_scatter.
constexpr int RADIX_ITEMS = 16;   // items per thread of a 256-thread tile: 4096 keys

// hist[digit * ntiles + tile]
template <class K>
__global__ void __launch_bounds__(256) radix_hist(const K* __restrict__ keys, int n, int shift, int ntiles, int* __restrict__ hist)
{
	using U = std::make_unsigned_t<K>;
	__shared__ int h[256];
	h[threadIdx.x] = 0;
	__syncthreads();
	const int base = blockIdx.x * 256 * RADIX_ITEMS;
	for (int j = 0; j < RADIX_ITEMS; j++) {
		const int i = base + j * 256 + threadIdx.x;
		if (i < n) atomicAdd(&h[(int)(((U)keys[i] >> shift) & 255)], 1);
	}
	__syncthreads();
	hist[threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// stable scatter: items keep their order within a digit (rounds in order, waves in order, lanes in order)
template <class K>
__global__ void __launch_bounds__(256) radix_scatter(const K* __restrict__ keys, const int* __restrict__ vals, int n, int shift,
                                                     int ntiles, const int* __restrict__ offs, K* __restrict__ okeys,
                                                     int* __restrict__ ovals)
{
	using U = std::make_unsigned_t<K>;
	__shared__ int base[256];
	__shared__ int wcnt[4][256];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	base[threadIdx.x] = offs[threadIdx.x * ntiles + blockIdx.x];
	for (int w = 0; w < 4; w++) wcnt[w][threadIdx.x] = 0;
	__syncthreads();
	const int tile = blockIdx.x * 256 * RADIX_ITEMS;
	const uint64_t lt = (1ull << lane) - 1;
	for (int j = 0; j < RADIX_ITEMS; j++) {
		const int i = tile + j * 256 + threadIdx.x;
		const bool valid = i < n;
		const K key = valid ? keys[i] : K(0);
		const int digit = (int)(((U)key >> shift) & 255);
		uint64_t peers = __ballot(valid);
		for (int b = 0; b < 8; b++) {
			const uint64_t m = __ballot(valid && ((digit >> b) & 1));
			peers &= ((digit >> b) & 1) ? m : ~m;
		}
		const int rank = __popcll(peers & lt);
		if (valid && (peers >> lane) == 1) wcnt[wave][digit] = __popcll(peers);   // the digit's last lane in this wave
		__syncthreads();
		if (valid) {
			int pos = base[digit] + rank;
			for (int w = 0; w < wave; w++) pos += wcnt[w][digit];
			okeys[pos] = key;
			ovals[pos] = vals[i];
		}
		__syncthreads();
		base[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
		for (int w = 0; w < 4; w++) wcnt[w][threadIdx.x] = 0;
		__syncthreads();
	}
}

// the sort's second key / value pair, the digit-major histogram, its scan and the scan's partial sums
template <class K>
struct SortBufs {
	K* k1;
	int* v1;
	int *hist, *offs, *part;
};
int sort_tiles(int n) { return (n + 256 * RADIX_ITEMS - 1) / (256 * RADIX_ITEMS); }
// the buffers for sorting n items; `part` is long enough for a scan of `scan_n` values too, for callers that reuse it
template <class K>
SortBufs<K> sort_take(Arena& ws, int n, long long scan_n = 0)
{
	const long long nh = 256LL * sort_tiles(n);
	SortBufs<K> b;
	b.k1 = ws.take<K>(n); b.v1 = ws.take<int>(n); b.hist = ws.take<int>(nh); b.offs = ws.take<int>(nh + 1);
	b.part = ws.take<int>(scan_part_len(nh > scan_n ? nh : scan_n));
	return b;
}
// sorts (k0, v0) by the low `bits` bits of the keys, stably, in ceil(bits / 8) passes; the result ends up in k0 / v0, which
// trade places with b.k1 / b.v1 after every pass
template <class K>
int radix_sort(K*& k0, int*& v0, int n, int bits, SortBufs<K>& b, hipStream_t s)
{
	const int ntiles = sort_tiles(n);
	for (int shift = 0; shift < bits; shift += 8) {
		hipLaunchKernelGGL(radix_hist<K>, dim3(ntiles), dim3(256), 0, s, k0, n, shift, ntiles, b.hist);
		const int rc = exclusive_scan<int>(b.hist, 256 * ntiles, b.offs, b.part, s);
		if (rc) return rc;
		hipLaunchKernelGGL(radix_scatter<K>, dim3(ntiles), dim3(256), 0, s, k0, v0, n, shift, ntiles, b.offs, b.k1, b.v1);
		K* tk = k0; k0 = b.k1; b.k1 = tk;
		int* tv = v0; v0 = b.v1; b.v1 = tv;
	}
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // namespace

#endif  // GSR_SORT_H_INCLUDED
