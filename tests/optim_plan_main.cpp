// The host-side planning code of the optimiser (gaustudio_amd/csrc/gsr_optim_plan.h) in a stand-alone program, for
// tests/test_optim_model.py to build with -fsanitize=address,undefined and run: threshold rounding, the constants of an Adam
// step, the row limits and the sizes that follow from the totals of a classify pass.  It prints what it computed; the test
// compares with tests/optim_model.py.
#include <limits.h>
#include <stdio.h>

#include <vector>

#include "gsr_optim_plan.h"

using namespace optim_plan;

int main()
{
	Thresholds t;
	if (!thresholds(0.01, 4.0, 0.05, 2, &t)) return 1;
	printf("thresholds %a %a %a %a\n", t.t_big, t.t_world, t.t_op, t.d_split);
	if (!thresholds(0.01, 4.0, 0.0, 2, &t)) return 1;
	printf("thresholds0 %a %a %a %a\n", t.t_big, t.t_world, t.t_op, t.d_split);
	// what must be refused: no extent, an opacity of one, no children, too many, a NaN
	if (thresholds(0.01, 0.0, 0.05, 2, &t) || thresholds(0.01, 4.0, 1.0, 2, &t) || thresholds(0.01, 4.0, 0.05, 0, &t) ||
	    thresholds(0.01, 4.0, 0.05, MAX_SPLIT + 1, &t) || thresholds(0.0, 4.0, 0.05, 2, &t) ||
	    thresholds(0.01, __builtin_nan(""), 0.05, 2, &t))
		return 2;

	AdamConsts c;
	if (!adam_consts(1.6e-4, 0.9, 0.999, 1000, &c)) return 3;
	printf("adam1000 %a %a %a %a\n", c.c1, c.c2, c.sqrt_bc2, c.step_size);
	if (!adam_consts(5e-2, 0.9, 0.999, 1, &c)) return 3;
	printf("adam1 %a %a %a %a\n", c.c1, c.c2, c.sqrt_bc2, c.step_size);
	if (adam_consts(1e-3, 0.9, 0.999, 0, &c) || adam_consts(-1.0, 0.9, 0.999, 1, &c) || adam_consts(1e-3, 1.0, 0.999, 1, &c) ||
	    adam_consts(__builtin_nan(""), 0.9, 0.999, 1, &c) || adam_consts(__builtin_inf(), 0.9, 0.999, 1, &c))
		return 4;
	if (!adam_consts(0.0, 0.9, 0.999, LLONG_MAX, &c) || c.step_size != 0.f || c.sqrt_bc2 != 1.f) return 5;

	const long long limit = ROW_LIMIT / MAX_WIDTH + 1;   // the first row count that is refused
	printf("rows %d %d %d %d\n", (int)rows_ok(0), (int)rows_ok(limit - 1), (int)rows_ok(limit), (int)rows_ok(-1));
	if (rows_ok((long long)INT_MAX) || rows_ok(LLONG_MAX / MAX_WIDTH)) return 6;

	const int a[3] = {10, 5, 7}, b[3] = {(int)limit, 0, 0}, d[3] = {(int)limit - 1, 0, 0}, e[3] = {-1, 0, 0};
	const int big[3] = {INT_MAX, INT_MAX, INT_MAX};
	printf("after %lld %lld %lld %lld %lld\n", rows_after(a, 3), rows_after(b, 1), rows_after(d, 1), rows_after(e, 1), rows_after(a, 0));
	if (rows_after(big, MAX_SPLIT) != -1) return 7;

	// the allocation sizes that follow from the totals: one row buffer per group width, written to its last element
	const int widths[6] = {3, 3, 45, 1, 3, 4};
	const long long n_after = rows_after(a, 3);
	for (int w : widths) {
		std::vector<float> rows((size_t)n_after * w);
		rows[rows.size() - 1] = 1.f;
		std::vector<int> pos(3 * (size_t)(a[0] + a[1] + a[2]) + 1);
		pos[pos.size() - 1] = (int)n_after;
		if (rows.back() != 1.f || pos.back() != 36) return 8;
	}
	printf("units %u %u %u %u %u %u\n", units_of(0, 0), units_of(1, 0), units_of(4, 0), units_of(5, 0), units_of(4, 1), units_of(8, 3));
	if (units_of(0xFFFFFFFFu, 3) != 0x40000001u) return 9;
	return 0;
}
