// q6codes.h -- the fused Q6's predicate bounds in the code domain of a column
// image (plain host C++, no HIP: tests compile it alone).
//
// An image of width w (1 | 2 bytes) holds code = value - base for the codes
// 0 .. 2^(8w) - 2; the all-ones code is nil.  The bounds below select
// exactly the codes whose VALUE passes the raw predicate, for any int64
// bound: below the base, above the largest code, INT64_MIN / INT64_MAX, or
// a reversed pair.  The differences are taken in 128 bits, so nothing here
// can overflow; the nil code is above every bound returned, so nils fail
// the code predicate as they fail the raw one.
#pragma once

#include <cstdint>

// [*clo, *chi]: the codes c with lo <= base + c <= hi (none: *clo = 1, *chi = 0)
inline void
q6_code_range(int64_t base, int width, int64_t lo, int64_t hi, uint32_t *clo, uint32_t *chi)
{
	const __int128 maxc = ((__int128) 1 << (8 * width)) - 2;
	__int128 l = (__int128) lo - (__int128) base, h = (__int128) hi - (__int128) base;
	if (l < 0)
		l = 0;
	if (h > maxc)
		h = maxc;
	if (l > h) {
		*clo = 1;
		*chi = 0;
		return;
	}
	*clo = (uint32_t) l;
	*chi = (uint32_t) h;
}

// k: the codes c with base + c < bound are exactly those with c < k
inline uint32_t
q6_code_below(int64_t base, int width, int64_t bound)
{
	const __int128 maxc = ((__int128) 1 << (8 * width)) - 2;
	__int128 k = (__int128) bound - (__int128) base;
	if (k < 0)
		k = 0;
	if (k > maxc + 1)
		k = maxc + 1;
	return (uint32_t) k;
}

// The same for a packed image (q6pack.h): value = base + stride * code, codes
// 0 .. 2^wbits - 2, stride >= 1.  Lower bounds round up, upper bounds round
// down, so a bound off the stride selects exactly the values inside it.

// [*clo, *chi]: the codes c with lo <= base + stride * c <= hi (none: *clo = 1, *chi = 0)
inline void
q6_pcode_range(int64_t base, uint64_t stride, int wbits, int64_t lo, int64_t hi, uint32_t *clo, uint32_t *chi)
{
	const __int128 maxc = ((__int128) 1 << wbits) - 2, st = (__int128) stride;
	__int128 l = (__int128) lo - (__int128) base, h = (__int128) hi - (__int128) base;
	l = l <= 0 ? 0 : (l + st - 1) / st;
	h = h < 0 ? -1 : h / st;
	if (h > maxc)
		h = maxc;
	if (l > h) {
		*clo = 1;
		*chi = 0;
		return;
	}
	*clo = (uint32_t) l;
	*chi = (uint32_t) h;
}

// [clo, chi] as the kernel tests it, with one unsigned compare: c - *plo <=
// *pspan.  An empty range becomes *plo = 2^16, above every code and the nil
// code of every width, with *pspan = 0.
inline void
q6_pcode_window(uint32_t clo, uint32_t chi, uint32_t *plo, uint32_t *pspan)
{
	const bool none = clo > chi;
	*plo = none ? 0x10000u : clo;
	*pspan = none ? 0 : chi - clo;
}

// k: the codes c with base + stride * c < bound are exactly those with c < k
// (k <= 2^wbits - 1, the nil code, which therefore never passes)
inline uint32_t
q6_pcode_below(int64_t base, uint64_t stride, int wbits, int64_t bound)
{
	const __int128 maxc = ((__int128) 1 << wbits) - 2, st = (__int128) stride;
	__int128 k = (__int128) bound - (__int128) base;
	k = k <= 0 ? 0 : (k + st - 1) / st;
	if (k > maxc + 1)
		k = maxc + 1;
	return (uint32_t) k;
}
