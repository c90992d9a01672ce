// Stand-alone check of the fused Q6's date predicate in the code domain of a
// shipdate image (built and run by tests/test_q6_dates.py, with
// -fsanitize=undefined where the compiler has it).  mgdk_q6_fused turns
// sd >= d0 && sd < d1 into q6_code_range(base, width, d0, (int64_t) d1 - 1):
// for every width, a set of int bases and every pair of int bounds from a
// dense edge set (the ends of the int range, values around the base and
// around the largest code), that range must select exactly the codes whose
// value passes the raw predicate; the nil code passes for no pair.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../monetdb_amd/csrc/q6codes.h"

int
main()
{
	long checked = 0, bad = 0;
	// a column's base is its smallest non-nil value: any int above INT32_MIN
	const int64_t bases[] = {0, 1, -1, 100, -40000, 2060000, INT32_MIN + 1, INT32_MIN + 2, INT32_MIN + 300,
				 (int64_t) INT32_MAX - 254, (int64_t) INT32_MAX - 65534, (int64_t) INT32_MAX - 300,
				 (int64_t) INT32_MAX - 70000, INT32_MAX, (int64_t) INT32_MAX - 1};
	for (int width = 1; width <= 2; width++) {
		const int64_t maxc = ((int64_t) 1 << (8 * width)) - 2;
		for (int64_t base : bases) {
			std::vector<int32_t> bounds = {INT32_MIN, INT32_MIN + 1, INT32_MIN + 2, INT32_MAX, INT32_MAX - 1, 0, -1, 1};
			for (int d = -3; d <= 3; d++) {
				const int64_t near[] = {base + d, base + maxc + d, base + maxc / 2 + d};
				for (int64_t v : near)
					if (v >= INT32_MIN && v <= INT32_MAX)
						bounds.push_back((int32_t) v);
			}
			// both ends, the middle, and the nil code
			const int64_t codes[] = {0, 1, 2, 3, maxc / 2 - 1, maxc / 2, maxc / 2 + 1, maxc - 3, maxc - 2, maxc - 1,
						 maxc, maxc + 1};
			for (int32_t d0 : bounds) {
				for (int32_t d1 : bounds) {
					uint32_t clo, chi;
					q6_code_range(base, width, d0, (int64_t) d1 - 1, &clo, &chi);
					for (int64_t c : codes) {
						const bool nil = c == maxc + 1;
						const int64_t v = base + c;
						if (!nil && v > INT32_MAX)
							continue;  // an image never holds a code beyond the int range
						const bool raw = !nil && v >= d0 && v < d1;
						checked++;
						if (raw != ((uint32_t) c >= clo && (uint32_t) c <= chi)) {
							bad++;
							printf("width %d base %lld [%d, %d) code %lld -> [%u, %u]\n", width, (long long) base,
							       d0, d1, (long long) c, clo, chi);
						}
					}
				}
			}
		}
	}
	printf("%ld checked, %ld wrong\n", checked, bad);
	return bad ? 1 : 0;
}
