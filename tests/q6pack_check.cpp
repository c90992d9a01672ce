// Stand-alone check of the packed column images' host arithmetic (built and
// run by tests/test_q6_packed.py, with -fsanitize=undefined where the
// compiler has it).
//
// 1. q6_pcode_range / q6_pcode_below / q6_pcode_window (q6codes.h): for small
//    bases, strides 1 .. 7 and 100, all four widths and every bound in a
//    window around the code range plus the ends of the int64 range, the code
//    bounds must select exactly the codes whose value base + stride * code
//    passes the raw predicate, in the one-compare form the kernel uses; the
//    nil code passes for no bound.
// 2. q6p_pack8 / q6p_code (q6pack.h): packing groups of 8 codes and reading
//    them back gives the codes, for every width, the nil code and the rows at
//    a chunk's edges included, and the words are the little-endian bit string
//    with row r at bit r * wbits.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../monetdb_amd/csrc/q6codes.h"
#include "../monetdb_amd/csrc/q6pack.h"

static long checked = 0, bad = 0;

static void
check_bounds(int64_t base, uint64_t stride, int wbits)
{
	const int64_t maxc = ((int64_t) 1 << wbits) - 2;
	std::vector<int64_t> codes;
	if (wbits <= 8) {
		for (int64_t c = 0; c <= maxc + 1; c++)
			codes.push_back(c);
	} else {
		const int64_t pick[] = {0, 1, 2, 3, maxc / 2 - 1, maxc / 2, maxc / 2 + 1, maxc - 2, maxc - 1, maxc, maxc + 1};
		codes.assign(pick, pick + sizeof(pick) / sizeof(pick[0]));
	}
	// bounds: on, and up to a stride either side of, the values of the codes
	// around both ends and the middle, two strides beyond each end, the ends of int64
	std::vector<int64_t> bounds = {INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1, 0, -1, 1};
	const int64_t around[] = {-2, -1, 0, 1, 2, maxc / 2, maxc - 2, maxc - 1, maxc, maxc + 1, maxc + 2, maxc + 3};
	const int64_t step = stride > 7 ? (int64_t) stride / 4 + 1 : 1;
	for (int64_t c : around) {
		for (int64_t d = -(int64_t) (stride > 1000 ? 2 : stride); d <= (int64_t) (stride > 1000 ? 2 : stride); d += step) {
			const __int128 v = (__int128) base + (__int128) stride * c + d;
			if (v >= INT64_MIN && v <= INT64_MAX)
				bounds.push_back((int64_t) v);
		}
	}
	for (int64_t lo : bounds) {
		// quantity < bound
		const uint32_t k = q6_pcode_below(base, stride, wbits, lo);
		uint32_t blo, bspan;
		if (k == 0)
			q6_pcode_window(1, 0, &blo, &bspan);
		else
			q6_pcode_window(0, k - 1, &blo, &bspan);
		for (int64_t c : codes) {
			const bool nil = c == maxc + 1;
			const __int128 v = (__int128) base + (__int128) stride * c;
			const bool raw = !nil && v < lo;
			checked++;
			if (raw != ((uint32_t) c < k) || raw != ((uint32_t) c - blo <= bspan) || k > (uint32_t) maxc + 1) {
				bad++;
				printf("below: base %lld stride %llu wbits %d bound %lld code %lld -> k %u\n", (long long) base,
				       (unsigned long long) stride, wbits, (long long) lo, (long long) c, k);
			}
		}
		for (int64_t hi : bounds) {
			uint32_t clo, chi, plo, pspan;
			q6_pcode_range(base, stride, wbits, lo, hi, &clo, &chi);
			q6_pcode_window(clo, chi, &plo, &pspan);
			const bool ordered = clo > chi || chi <= (uint32_t) maxc;
			for (int64_t c : codes) {
				const bool nil = c == maxc + 1;
				const __int128 v = (__int128) base + (__int128) stride * c;
				const bool raw = !nil && v >= lo && v <= hi;
				checked++;
				if (!ordered || raw != ((uint32_t) c >= clo && (uint32_t) c <= chi) || raw != ((uint32_t) c - plo <= pspan)) {
					bad++;
					printf("range: base %lld stride %llu wbits %d [%lld, %lld] code %lld -> [%u, %u]\n", (long long) base,
					       (unsigned long long) stride, wbits, (long long) lo, (long long) hi, (long long) c, clo, chi);
				}
			}
		}
	}
}

// bit string: row r's code at bit r * wbits, little-endian
static uint32_t
bitstring_code(const std::vector<uint32_t> &words, uint64_t r, int wbits)
{
	const uint8_t *bytes = (const uint8_t *) words.data();
	uint32_t v = 0;
	for (int b = 0; b < wbits; b++) {
		const uint64_t bit = r * (uint64_t) wbits + (uint64_t) b;
		v |= (uint32_t) ((bytes[bit >> 3] >> (bit & 7)) & 1u) << b;
	}
	return v;
}

template <int WB>
static void
check_pack()
{
	const uint64_t n = 2 * Q6P_CH + 77;          // two full chunks and a part of a third
	const uint64_t bytes = q6p_bytes(n, WB);
	checked++;
	if (bytes != 3 * (uint64_t) (Q6P_CH / 8) * WB || q6p_bytes(Q6P_CH, WB) != (uint64_t) (Q6P_CH / 8) * WB ||
	    q6p_bytes(1, WB) != (uint64_t) (Q6P_CH / 8) * WB || q6p_nil(WB) != (1u << WB) - 1) {
		bad++;
		printf("pack: wbits %d: %llu bytes for %llu rows\n", WB, (unsigned long long) bytes, (unsigned long long) n);
	}
	const uint64_t rows = bytes * 8 / WB, groups = rows / Q6P_ROWS;
	std::vector<uint32_t> want(rows), words(bytes / 4, 0xdeadbeefu);
	uint64_t s = 0x9e3779b97f4a7c15ull * WB;
	for (uint64_t r = 0; r < rows; r++) {
		s = s * 6364136223846793005ull + 1442695040888963407ull;
		want[r] = r >= n ? q6p_nil(WB) : (uint32_t) (s >> 40) & q6p_nil(WB);
	}
	// the ends of the code range and the nil code at the edges of groups and chunks
	const uint64_t edges[] = {0, 1, 7, 8, Q6P_CH - 1, Q6P_CH, Q6P_CH + 1, 2 * Q6P_CH - 1, 2 * Q6P_CH};
	const uint32_t ends[] = {q6p_nil(WB), q6p_nil(WB) - 1, 0};
	int e = 0;
	for (uint64_t r : edges)
		want[r] = ends[e++ % 3];
	for (uint64_t g = 0; g < groups; g++) {
		const uint64_t off = q6p_group_offset(g, WB);
		checked++;
		if (off % 4 != 0 || off + WB > bytes) {
			bad++;
			printf("pack: wbits %d group %llu at byte %llu\n", WB, (unsigned long long) g, (unsigned long long) off);
			continue;
		}
		q6p_pack8<WB>(&want[g * Q6P_ROWS], &words[off / 4]);
	}
	for (uint64_t r = 0; r < rows; r++) {
		const uint64_t g = r / Q6P_ROWS;
		const uint32_t got = q6p_code<WB>(&words[q6p_group_offset(g, WB) / 4], (int) (r % Q6P_ROWS));
		checked++;
		if (got != want[r] || bitstring_code(words, r, WB) != want[r]) {
			bad++;
			printf("pack: wbits %d row %llu: %u, bit string %u, want %u\n", WB, (unsigned long long) r, got,
			       bitstring_code(words, r, WB), want[r]);
		}
	}
}

int
main()
{
	const int64_t bases[] = {0, 1, -1, 100, -7, 5};
	const uint64_t strides[] = {1, 2, 3, 4, 5, 6, 7, 100};
	const int widths[] = {4, 8, 12, 16};
	for (int wbits : widths)
		for (int64_t base : bases)
			for (uint64_t stride : strides)
				check_bounds(base, stride, wbits);
	// a base and a stride at the ends of the range: nothing may overflow
	check_bounds(INT64_MIN + 1, 1, 16);
	check_bounds(INT64_MAX - 14, 1, 4);
	check_bounds(INT64_MIN + 1, (uint64_t) 1 << 59, 4);
	check_pack<4>();
	check_pack<8>();
	check_pack<12>();
	check_pack<16>();
	checked += q6p_width(14) == 4 && q6p_width(15) == 8 && q6p_width(254) == 8 && q6p_width(255) == 12 &&
		   q6p_width(4094) == 12 && q6p_width(4095) == 16 && q6p_width(65534) == 16 && q6p_width(65535) == 0 &&
		   q6p_width(0) == 4;
	if (!(q6p_width(14) == 4 && q6p_width(15) == 8 && q6p_width(254) == 8 && q6p_width(255) == 12 &&
	      q6p_width(4094) == 12 && q6p_width(4095) == 16 && q6p_width(65534) == 16 && q6p_width(65535) == 0 &&
	      q6p_width(0) == 4)) {
		bad++;
		printf("q6p_width\n");
	}
	printf("%ld checked, %ld wrong\n", checked, bad);
	return bad ? 1 : 0;
}
