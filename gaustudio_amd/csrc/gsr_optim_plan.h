// gsr_optim_plan.h -- the host-side planning of the optimiser and of density control (gsr_optim.hip): the float32 constants
// of an Adam step, the decision thresholds of a densification, the row limits and the sizes that follow from the totals of a
// classify pass.  Plain C++ with no HIP in it, so that tests/optim_plan_main.cpp can run it under the host sanitizers.
// Every constant is formed in float64 and rounded to float32 once (restated in tests/optim_model.py).
#ifndef GSR_OPTIM_PLAN_H_INCLUDED
#define GSR_OPTIM_PLAN_H_INCLUDED
#include <math.h>

namespace optim_plan {

constexpr int MAX_WIDTH = 45;                 // floats of the widest group's row: f_rest with K = 15
constexpr long long ROW_LIMIT = 1LL << 31;    // rows * MAX_WIDTH stays below it
constexpr int MAX_SPLIT = 8;

inline bool rows_ok(long long n) { return n >= 0 && n * MAX_WIDTH < ROW_LIMIT; }

struct AdamConsts { float c1, c2, sqrt_bc2, step_size; };   // 1 - beta1, 1 - beta2, sqrt(1 - beta2^t), lr / (1 - beta1^t)

inline bool adam_consts(double lr, double beta1, double beta2, long long step, AdamConsts* out)
{
	if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || step < 1 || !isfinite(lr)) return false;
	const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
	out->c1 = (float)(1.0 - beta1);
	out->c2 = (float)(1.0 - beta2);
	out->sqrt_bc2 = (float)sqrt(bc2);
	out->step_size = (float)(lr / bc1);
	return true;
}

struct Thresholds { float t_big, t_world, t_op, d_split; };

// t_big = log(percent_dense extent), t_world = log(0.1 extent), t_op = logit(min_opacity), d_split = log(0.8 n_split)
inline bool thresholds(double percent_dense, double extent, double min_opacity, int n_split, Thresholds* out)
{
	if (!(percent_dense > 0.0) || !(extent > 0.0) || !isfinite(percent_dense) || !isfinite(extent)) return false;
	if (!(min_opacity >= 0.0 && min_opacity < 1.0) || n_split < 1 || n_split > MAX_SPLIT) return false;
	out->t_big = (float)log(percent_dense * extent);
	out->t_world = (float)log(0.1 * extent);
	out->t_op = (float)log(min_opacity / (1.0 - min_opacity));   // min_opacity = 0: -inf, nothing fails the test
	out->d_split = (float)log(0.8 * (double)n_split);
	return true;
}

// totals = {kept sources, clones, split sources whose children pass}: rows after the pass, or -1 beyond the limit
inline long long rows_after(const int totals[3], int n_split)
{
	if (totals[0] < 0 || totals[1] < 0 || totals[2] < 0 || n_split < 1 || n_split > MAX_SPLIT) return -1;
	const long long n = (long long)totals[0] + totals[1] + (long long)n_split * totals[2];
	return rows_ok(n) ? n : -1;
}

// 16-byte units of a tensor of n floats that starts `shift` floats past a 16-byte boundary
inline unsigned units_of(unsigned n, unsigned shift) { return n ? (unsigned)(((unsigned long long)n + shift + 3) / 4) : 0u; }

}  // namespace optim_plan

#endif  // GSR_OPTIM_PLAN_H_INCLUDED
