// q6pack.h -- the layout of a packed column image (Priv::pimg, runtime.hip):
// one definition for the encode kernel, the fused Q6 that reads it
// (q6p::k_q6s, tpch.hip) and the host check (tests/q6pack_check.cpp).  Plain
// C++: compiles for the host alone and for the device.
//
// code = (value - base) / stride in WB = 4 | 8 | 12 | 16 bits, the all-ones
// code is nil.  Row r's code sits at bit r * WB of a little-endian bit
// string, so the 8 rows 8g .. 8g+7 of group g are the WB / 4 dwords at byte
// g * WB (4-byte aligned), a 512-row chunk is 64 WB bytes and a 128-B line
// holds 1024 / WB rows.  The heap is padded to whole chunks.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define Q6P_HD __host__ __device__ __forceinline__
#else
#define Q6P_HD inline
#endif

constexpr unsigned Q6P_CH = 512;      // rows per chunk
constexpr unsigned Q6P_ROWS = 8;      // rows per group (one lane of the reader, one thread of the encoder)

// smallest of the four widths that holds the codes 0 .. maxcode below its nil code; 0: none
Q6P_HD int
q6p_width(uint64_t maxcode)
{
	return maxcode <= 14 ? 4 : maxcode <= 254 ? 8 : maxcode <= 4094 ? 12 : maxcode <= 65534 ? 16 : 0;
}

Q6P_HD uint32_t
q6p_nil(int wbits)
{
	return (1u << wbits) - 1;
}

// bytes of an image of n rows: whole chunks
Q6P_HD uint64_t
q6p_bytes(uint64_t n, int wbits)
{
	return (n + Q6P_CH - 1) / Q6P_CH * (Q6P_CH / 8) * (uint64_t) wbits;
}

// byte offset of the dwords of group g (rows 8g .. 8g+7)
Q6P_HD uint64_t
q6p_group_offset(uint64_t g, int wbits)
{
	return g * (uint64_t) wbits;
}

// code k (0 .. 7) of a group from its WB / 4 dwords
template <int WB>
Q6P_HD uint32_t
q6p_code(const uint32_t *w, int k)
{
	static_assert(WB == 4 || WB == 8 || WB == 12 || WB == 16, "packed widths");
	const int bit = k * WB, d = bit >> 5, s = bit & 31;
	uint32_t v = w[d] >> s;
	if (s + WB > 32)                  // WB == 12 only: codes 2 and 5 straddle two dwords
		v |= w[d + 1] << (32 - s);
	return v & ((1u << WB) - 1);
}

// the WB / 4 dwords of a group from its 8 codes (each below 2^WB)
template <int WB>
Q6P_HD void
q6p_pack8(const uint32_t *c, uint32_t *w)
{
	static_assert(WB == 4 || WB == 8 || WB == 12 || WB == 16, "packed widths");
	for (int d = 0; d < WB / 4; d++)
		w[d] = 0;
	for (int k = 0; k < 8; k++) {
		const int bit = k * WB, d = bit >> 5, s = bit & 31;
		w[d] |= c[k] << s;
		if (s + WB > 32)
			w[d + 1] |= c[k] >> (32 - s);
	}
}
