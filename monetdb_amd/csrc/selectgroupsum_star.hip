// selectgroupsum_star.hip -- mgdk_select_groupsum_star_fused: the hashed
// fused select cascade + GROUP BY sums with predicate, key and factor columns
// of dimension tables reached through join indexes (a star join).  Kernel and
// entry are in selectgroupsum_hash.h, instantiated here with the gather
// (DESIGN.md 11.13).
#include "selectgroupsum_hash.h"

using namespace mgdk;

namespace {
thread_local unsigned long long st_last_lines = 0, st_last_gathers = 0;
}

extern "C" {

int
mgdk_select_groupsum_star_fused(const mgdk_selpred *preds, int npreds, mgdk_bat *s, mgdk_bat *const *keys, int nkeys,
				const mgdk_gsumexpr *sums, int nsums, const mgdk_starvia *vias, int nvias, int maxgroups,
				int *ngroups, mgdk_gsgroupw *groups, void *sumres, uint64_t *nonnil)
{
	return gh_entry<true>(preds, npreds, s, keys, nkeys, sums, nsums, vias, nvias, maxgroups, ngroups, groups, sumres,
			      nonnil, &st_last_lines, &st_last_gathers);
}

unsigned long long
mgdk_select_groupsum_star_last_lines(void)
{
	return st_last_lines;
}

unsigned long long
mgdk_select_groupsum_star_last_gathers(void)
{
	return st_last_gathers;
}

}  // extern "C"
