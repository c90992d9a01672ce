// selectgroupsum_hash.hip -- mgdk_select_groupsum_hash_fused: the fused
// select cascade + GROUP BY sums for keys of up to 8 bytes together and up to
// 256 groups, every column of one table.  Kernel and entry are in
// selectgroupsum_hash.h, instantiated here without the gather (DESIGN.md
// 11.12).
#include "selectgroupsum_hash.h"

using namespace mgdk;

namespace {
thread_local unsigned long long gh_last_lines = 0;
}

extern "C" {

int
mgdk_select_groupsum_hash_fused(const mgdk_selpred *preds, int npreds, mgdk_bat *s, mgdk_bat *const *keys, int nkeys,
				const mgdk_gsumexpr *sums, int nsums, int maxgroups, int *ngroups,
				mgdk_gsgroupw *groups, void *sumres, uint64_t *nonnil)
{
	unsigned long long gathers;              // none without the gather
	return gh_entry<false>(preds, npreds, s, keys, nkeys, sums, nsums, nullptr, 0, maxgroups, ngroups, groups, sumres,
			       nonnil, &gh_last_lines, &gathers);
}

unsigned long long
mgdk_select_groupsum_hash_last_lines(void)
{
	return gh_last_lines;
}

}  // extern "C"
