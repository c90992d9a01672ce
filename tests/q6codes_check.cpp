// Stand-alone check of q6codes.h (built and run by tests/test_q6_codes.py,
// with -fsanitize=undefined where the compiler has it): for every width,
// a set of bases and every pair of bounds from a set that holds the ends of
// the lng range, values around the base and around the largest code, the
// code-domain predicate must select exactly the codes whose value passes
// the raw predicate.  Values are compared in 128 bits here, so the check
// itself cannot overflow.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../monetdb_amd/csrc/q6codes.h"

int
main()
{
	long checked = 0, bad = 0;
	const int64_t bases[] = {0, 100, -3, -40000, INT64_MIN + 1, INT64_MIN + 2, -((int64_t) 1 << 62) + 11,
				 ((int64_t) 1 << 62) - 5000, INT64_MAX - 254, INT64_MAX - 65534, INT64_MAX - 300};
	for (int width = 1; width <= 2; width++) {
		const int64_t maxc = ((int64_t) 1 << (8 * width)) - 2;
		for (int64_t base : bases) {
			if ((__int128) base + maxc > INT64_MAX)
				continue;          // an image never holds a code beyond the lng range
			std::vector<int64_t> bounds = {INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1, 0, 5, 7, 2400, -1};
			for (int d = -2; d <= 2; d++) {
				const __int128 near[] = {(__int128) base + d, (__int128) base + maxc + d,
							 (__int128) base + maxc / 2 + d};
				for (__int128 v : near)
					if (v >= INT64_MIN && v <= INT64_MAX)
						bounds.push_back((int64_t) v);
			}
			// the codes worth looking at: both ends, the middle, and the nil code
			const int64_t codes[] = {0, 1, 2, maxc / 2 - 1, maxc / 2, maxc / 2 + 1, maxc - 2, maxc - 1, maxc,
						 maxc + 1};
			for (int64_t lo : bounds) {
				const uint32_t k = q6_code_below(base, width, lo);
				for (int64_t c : codes) {
					const bool nil = c == maxc + 1;
					const bool raw = !nil && (__int128) base + c < (__int128) lo;
					checked++;
					if (raw != ((uint32_t) c < k)) {
						bad++;
						printf("below: width %d base %lld bound %lld code %lld k %u\n", width,
						       (long long) base, (long long) lo, (long long) c, k);
					}
				}
				for (int64_t hi : bounds) {
					uint32_t clo, chi;
					q6_code_range(base, width, lo, hi, &clo, &chi);
					for (int64_t c : codes) {
						const bool nil = c == maxc + 1;
						const __int128 v = (__int128) base + c;
						const bool raw = !nil && v >= lo && v <= hi;
						checked++;
						if (raw != ((uint32_t) c >= clo && (uint32_t) c <= chi)) {
							bad++;
							printf("range: width %d base %lld [%lld, %lld] code %lld -> [%u, %u]\n", width,
							       (long long) base, (long long) lo, (long long) hi, (long long) c, clo,
							       chi);
						}
					}
				}
			}
		}
	}
	printf("%ld checked, %ld wrong\n", checked, bad);
	return bad ? 1 : 0;
}
