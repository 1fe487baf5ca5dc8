// gsr_anchor_plan.h -- the host-side planning of anchor control (gsr_anchor.hip): the size limits, the range a voxel cell may
// have, and the sort key of a level -- three cell coordinates rebased to the smallest candidate cell and packed x-major into as
// few bits as the occupied range needs.  Plain C++ without HIP, so that tests/anchor_plan_main.cpp can run it under the host
// sanitizers.
#ifndef GSR_ANCHOR_PLAN_H_INCLUDED
#define GSR_ANCHOR_PLAN_H_INCLUDED
#include <stdint.h>

#ifdef __HIPCC__
#define ANCHOR_HD __host__ __device__
#else
#define ANCHOR_HD
#endif

namespace anchor_plan {

constexpr int CELL_MIN = -(1 << 20), CELL_MAX = (1 << 20) - 1;   // a signed 21-bit field
constexpr long long MAX_ANCHORS = 1LL << 24;
constexpr int MAX_OFFSETS = 16;
constexpr long long SLOT_LIMIT = 1LL << 31;                       // anchors * k stays below it

inline bool sizes_ok(long long n, long long k)
{
	return k >= 1 && k <= MAX_OFFSETS && n >= 0 && n <= MAX_ANCHORS && n * k < SLOT_LIMIT;
}

inline int span_bits(long long n)   // bits to hold the values 0 .. n - 1 (gsr_ws.h bits_for)
{
	int b = 1;
	while (b < 62 && (1LL << b) < n) b++;
	return b;
}

struct KeyPlan {
	int lo[3];      // the smallest candidate cell per axis
	int hi[3];
	int shift[3];   // x-major: ascending keys are the lexicographic (x, y, z) order
	int bits;       // of the whole key: the sort runs ceil(bits / 8) passes
};

// false for an empty or out-of-range box
inline bool key_plan(const int lo[3], const int hi[3], KeyPlan* p)
{
	int w[3];
	for (int c = 0; c < 3; c++) {
		if (lo[c] > hi[c] || lo[c] < CELL_MIN || hi[c] > CELL_MAX) return false;
		p->lo[c] = lo[c];
		p->hi[c] = hi[c];
		w[c] = span_bits((long long)hi[c] - lo[c] + 1);
	}
	p->shift[2] = 0;
	p->shift[1] = w[2];
	p->shift[0] = w[2] + w[1];
	p->bits = w[0] + w[1] + w[2];
	return true;
}

ANCHOR_HD inline uint64_t pack_key(const KeyPlan& p, int x, int y, int z)
{
	return ((uint64_t)(uint32_t)(x - p.lo[0]) << p.shift[0]) | ((uint64_t)(uint32_t)(y - p.lo[1]) << p.shift[1]) |
	       (uint64_t)(uint32_t)(z - p.lo[2]);
}

ANCHOR_HD inline void unpack_key(const KeyPlan& p, uint64_t key, int cell[3])
{
	cell[0] = (int)(key >> p.shift[0]) + p.lo[0];
	cell[1] = (int)((key >> p.shift[1]) & ((1ull << (p.shift[0] - p.shift[1])) - 1)) + p.lo[1];
	cell[2] = (int)(key & ((1ull << p.shift[1]) - 1)) + p.lo[2];
}

}  // namespace anchor_plan

#endif  // GSR_ANCHOR_PLAN_H_INCLUDED
