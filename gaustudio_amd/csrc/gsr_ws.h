// gsr_ws.h -- the host scaffolding of the geometry modules (gsr_knn, gsr_mesh, gsr_mesh_clean, gsr_mesh_bake, gsr_voxel,
// gsr_psr): the workspace arena, the launch and key-width helpers, the status word and the HIP error macro.  Host code only,
// internal linkage, no kernels.
#ifndef GSR_WS_H_INCLUDED
#define GSR_WS_H_INCLUDED
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/gsrast.h"

#define GSR_TRY(expr) do { if ((expr) != hipSuccess) return GSR_ERR_HIP; } while (0)

namespace {

// Bump allocation out of one workspace block in 256-byte granules.  On a null block take() hands out nullptr and still
// advances `off`: the code that carves a block, run on a null arena first, is also what sizes it (ws_carve).
struct Arena {
	char* p;
	size_t off;
	template <class T> T* take(size_t n)
	{
		T* r = p ? reinterpret_cast<T*>(p + off) : nullptr;
		off += (n * sizeof(T) + 255) & ~(size_t)255;
		return r;
	}
};

char* ws_alloc(gsr_alloc_fn alloc, void* ctx, size_t bytes) { return alloc ? alloc(ctx, bytes) : nullptr; }

// One call of the caller's allocator for the buffers that `carve(Arena&)` takes: carve runs on a null arena for the byte
// count, then on the block.  It only takes (and stores the pointers); false = no block, carve's pointers are null.
template <class Carve> bool ws_carve(gsr_alloc_fn alloc, void* ctx, Carve&& carve)
{
	Arena ws{nullptr, 0};
	carve(ws);
	ws = Arena{ws_alloc(alloc, ctx, ws.off), 0};
	if (!ws.p) return false;
	carve(ws);
	return true;
}

unsigned blocks(long long n) { return (unsigned)((n + 255) / 256); }

int bits_for(long long n)   // bits to hold the values 0 .. n - 1
{
	int b = 1;
	while (b < 62 && (1LL << b) < n) b++;
	return b;
}

// the status word that kernels set with atomicOr on a bad index: read back, GSR_ERR_ARG when set
int read_status(const int* status, hipStream_t s)
{
	int st = 0;
	GSR_TRY(hipMemcpyAsync(&st, status, sizeof(int), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	return st ? GSR_ERR_ARG : GSR_OK;
}

}  // namespace

#endif  // GSR_WS_H_INCLUDED
