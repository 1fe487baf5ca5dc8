// The host-side planning code of anchor control (gaustudio_amd/csrc/gsr_anchor_plan.h) in a stand-alone program, for
// tests/test_anchor_model.py to build with -fsanitize=address,undefined and run: the size limits, the key layout for a cell
// range, and that packed keys order cells lexicographically and unpack to what was packed.  It prints what it computed.
#include <stdio.h>

#include <vector>

#include "gsr_anchor_plan.h"

using namespace anchor_plan;

int main()
{
	printf("sizes %d %d %d %d %d %d %d\n", (int)sizes_ok(0, 1), (int)sizes_ok(1LL << 24, 16), (int)sizes_ok((1LL << 24) + 1, 1),
	       (int)sizes_ok(10, 0), (int)sizes_ok(10, 17), (int)sizes_ok(5, 16), (int)sizes_ok(-1, 1));
	KeyPlan p;
	const int flo[3] = {CELL_MIN, CELL_MIN, CELL_MIN}, fhi[3] = {CELL_MAX, CELL_MAX, CELL_MAX};
	if (!key_plan(flo, fhi, &p)) return 1;
	printf("full %d %d %d %d\n", p.bits, p.shift[0], p.shift[1], p.shift[2]);
	if (pack_key(p, CELL_MAX, CELL_MAX, CELL_MAX) != (1ull << 63) - 1 || pack_key(p, CELL_MIN, CELL_MIN, CELL_MIN) != 0) return 2;
	const int lo[3] = {-3, 0, 10}, hi[3] = {4, 1, 100};
	if (!key_plan(lo, hi, &p)) return 1;
	printf("small %d %d %d %d\n", p.bits, p.shift[0], p.shift[1], p.shift[2]);
	// what must be refused: an empty box, a box beyond the 21-bit range
	const int blo[3] = {5, 0, 0}, bhi[3] = {4, 0, 0}, olo[3] = {CELL_MIN - 1, 0, 0}, ohi[3] = {0, 0, CELL_MAX + 1};
	KeyPlan q;
	if (key_plan(blo, bhi, &q) || key_plan(olo, fhi, &q) || key_plan(flo, ohi, &q)) return 3;

	// every cell of the small box: keys ascend exactly in lexicographic (x, y, z) order and unpack to their cell
	std::vector<uint64_t> keys;
	int order = 1, roundtrip = 1;
	for (int x = lo[0]; x <= hi[0]; x++)
		for (int y = lo[1]; y <= hi[1]; y++)
			for (int z = lo[2]; z <= hi[2]; z++) {
				const uint64_t key = pack_key(p, x, y, z);
				if (!keys.empty() && key <= keys.back()) order = 0;
				if (key >> p.bits) order = 0;
				keys.push_back(key);
				int c[3];
				unpack_key(p, key, c);
				if (c[0] != x || c[1] != y || c[2] != z) roundtrip = 0;
			}
	int c[3];
	const int one[3] = {7, 7, 7};
	if (!key_plan(one, one, &p)) return 1;            // a single cell: one bit per axis
	unpack_key(p, pack_key(p, 7, 7, 7), c);
	if (p.bits != 3 || c[0] != 7 || c[1] != 7 || c[2] != 7) roundtrip = 0;
	printf("order %d\nroundtrip %d\n", order, roundtrip);
	return 0;
}
