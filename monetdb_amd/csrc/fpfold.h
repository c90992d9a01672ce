// fpfold.h -- the states and ordered pairwise combines of the parallel form
// of the order-dependent float folds, shared by the grouped
// aggregates (aggr.hip, groupstats.hip) and the window functions
// (analytic_func.hip, analytic_stats.hip).
#pragma once

#include "mgdk_internal.h"

namespace mgdk {

// ---- float average: (a, c) + (b, d) -> a + (b - a) * (d / (c + d)), the
// weighted mean of the partial means; nil: a nil row seen without skip_nils
struct FAvg {
	double a;
	double c;
	int nil;
};

__device__ __forceinline__ FAvg
favg_comb(const FAvg &x, const FAvg &y)
{
	FAvg r;
	r.nil = x.nil | y.nil;
	if (x.c == 0) {
		r.a = y.a;
		r.c = y.c;
	} else if (y.c == 0) {
		r.a = x.a;
		r.c = x.c;
	} else {
		r.c = x.c + y.c;
		r.a = x.a + (y.a - x.a) * (y.c / r.c);
	}
	return r;
}

// ---- Welford moments: the pairwise update of Chan, Golub and LeVeque
// (n = na + nb, d = mean_b - mean_a: mean = mean_a + d nb / n,
// M2 = M2a + M2b + d^2 na nb / n, the co-moments alike).  The statistics are
// compiled without contraction (their sources switch it off after their
// includes), so mom_comb does so in its own body: the same bits wherever it
// is included from.
enum { ST_VAR = 0, ST_COV = 1, ST_COR = 2 };

struct MomState {
	double n, mean1, mean2, m2, down1, down2;   // m2: the co-moment (up) for ST_COR
};

template <int KIND>
__device__ __forceinline__ MomState
mom_comb(const MomState &a, const MomState &b)
{
#pragma clang fp contract(off)
	if (a.n == 0)
		return b;
	if (b.n == 0)
		return a;
	MomState r;
	r.n = a.n + b.n;
	const double f = b.n / r.n, d1 = b.mean1 - a.mean1, w = a.n * f;
	r.mean1 = a.mean1 + d1 * f;
	r.mean2 = r.down1 = r.down2 = 0;
	if (KIND == ST_VAR) {
		r.m2 = a.m2 + b.m2 + d1 * d1 * w;
	} else {
		const double d2 = b.mean2 - a.mean2;
		r.mean2 = a.mean2 + d2 * f;
		r.m2 = a.m2 + b.m2 + d1 * d2 * w;
		if (KIND == ST_COR) {
			r.down1 = a.down1 + b.down1 + d1 * d1 * w;
			r.down2 = a.down2 + b.down2 + d2 * d2 * w;
		}
	}
	return r;
}

template <int KIND>
__device__ __forceinline__ bool
mom_inf(const MomState &s)
{
	return __builtin_isinf(s.m2) || (KIND == ST_COR && (__builtin_isinf(s.down1) || __builtin_isinf(s.down2)));
}

}  // namespace mgdk
