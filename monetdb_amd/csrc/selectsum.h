// selectsum.h -- what the fused select-cascade kernels share (selectsum.hip:
// sums over the survivors; selectgroupsum.hip: the same grouped by small
// keys): the normalised predicate, its evaluation, the 4-rows-per-lane column
// loads of a 256-row chunk and the count of the 128-byte lines they touch,
// and the host-side column / predicate checks.  DESIGN.md 11.10, 11.11.
#pragma once
#include "mgdk_internal.h"
#include "selnorm.h"

namespace mgdk {
namespace {

constexpr int SS_MAXP = 4;

struct SsP {
	const char *col;          // the column at the first row of the range
	int w, mode, nil_matches;
	int count;                // first use of the column: its lines are counted here
	int64_t vl, vh, nil;
};

typedef unsigned int ssu4 __attribute__((ext_vector_type(4)));
typedef unsigned int ssu2 __attribute__((ext_vector_type(2)));

// 128-byte lines of a 256-row chunk of a column of width w touched by the
// lanes in b (lane l reads bytes [4wl, 4wl + 4w) of the chunk: 32 / w lanes
// share a line)
__device__ __forceinline__ uint32_t
ss_lines(int w, uint64_t b)
{
	switch (w) {
	case 8:
		b |= b >> 1;
		b |= b >> 2;
		return (uint32_t) __popcll(b & 0x1111111111111111ull);
	case 4:
		b |= b >> 1;
		b |= b >> 2;
		b |= b >> 4;
		return (uint32_t) __popcll(b & 0x0101010101010101ull);
	case 2:
		b |= b >> 1;
		b |= b >> 2;
		b |= b >> 4;
		b |= b >> 8;
		return (uint32_t) __popcll(b & 0x0001000100010001ull);
	default:
		return ((uint32_t) b != 0) + ((uint32_t) (b >> 32) != 0);
	}
}

// the four rows of each of U chunks of one column, sign-extended.  PLAIN:
// per-row loads of rows < rows[u] (unaligned heaps, the partial chunk);
// otherwise raw buffer loads through a descriptor over the chunk's 256 w
// bytes, dead lanes out of range (zeros, no memory access)
template <int U, bool PLAIN>
__device__ __forceinline__ void
ss_load(const char *col, int w, const uint64_t (&ch)[U], const uint32_t (&rows)[U], unsigned lane,
	const bool (&live)[U], int64_t (&v)[U][4])
{
	if constexpr (PLAIN) {
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const uint32_t r = 4 * lane + k;
				int64_t x = 0;
				if (live[u] && r < rows[u]) {
					const uint64_t i = ch[u] * 256 + r;
					switch (w) {
					case 8: x = ((const int64_t *) col)[i]; break;
					case 4: x = ((const int32_t *) col)[i]; break;
					case 2: x = ((const int16_t *) col)[i]; break;
					default: x = ((const int8_t *) col)[i]; break;
					}
				}
				v[u][k] = x;
			}
	} else {
		// dword3 0x00020000 is the gfx950 (CDNA3/4) descriptor layout whose
		// range check returns zeros for the dead lanes' out-of-range offset
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "ss_load: buffer descriptor word 3 is laid out for gfx942 / gfx950 only"
#endif
		constexpr unsigned DEAD = 0x80000000u;
		switch (w) {
		case 8: {
			ssu4 r0[U], r1[U];
#pragma unroll
			for (int u = 0; u < U; u++) {
				__amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *) (col + ch[u] * 2048),
											      (short) 0, 2048, 0x00020000);
				r0[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, live[u] ? 32u * lane : DEAD, 0, 0);
				r1[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, live[u] ? 32u * lane + 16u : DEAD, 0, 0);
			}
#pragma unroll
			for (int u = 0; u < U; u++) {
				v[u][0] = (int64_t) (((unsigned long long) r0[u].y << 32) | r0[u].x);
				v[u][1] = (int64_t) (((unsigned long long) r0[u].w << 32) | r0[u].z);
				v[u][2] = (int64_t) (((unsigned long long) r1[u].y << 32) | r1[u].x);
				v[u][3] = (int64_t) (((unsigned long long) r1[u].w << 32) | r1[u].z);
			}
			break;
		}
		case 4: {
			ssu4 r[U];
#pragma unroll
			for (int u = 0; u < U; u++) {
				__amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *) (col + ch[u] * 1024),
											      (short) 0, 1024, 0x00020000);
				r[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, live[u] ? 16u * lane : DEAD, 0, 0);
			}
#pragma unroll
			for (int u = 0; u < U; u++) {
				v[u][0] = (int32_t) r[u].x;
				v[u][1] = (int32_t) r[u].y;
				v[u][2] = (int32_t) r[u].z;
				v[u][3] = (int32_t) r[u].w;
			}
			break;
		}
		case 2: {
			ssu2 r[U];
#pragma unroll
			for (int u = 0; u < U; u++) {
				__amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *) (col + ch[u] * 512),
											      (short) 0, 512, 0x00020000);
				r[u] = __builtin_amdgcn_raw_buffer_load_b64(rs, live[u] ? 8u * lane : DEAD, 0, 0);
			}
#pragma unroll
			for (int u = 0; u < U; u++) {
				v[u][0] = (int16_t) (r[u].x & 0xffffu);
				v[u][1] = (int16_t) (r[u].x >> 16);
				v[u][2] = (int16_t) (r[u].y & 0xffffu);
				v[u][3] = (int16_t) (r[u].y >> 16);
			}
			break;
		}
		default: {
			unsigned int r[U];
#pragma unroll
			for (int u = 0; u < U; u++) {
				__amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *) (col + ch[u] * 256),
											      (short) 0, 256, 0x00020000);
				r[u] = __builtin_amdgcn_raw_buffer_load_b32(rs, live[u] ? 4u * lane : DEAD, 0, 0);
			}
#pragma unroll
			for (int u = 0; u < U; u++) {
				v[u][0] = (int8_t) (r[u] & 0xffu);
				v[u][1] = (int8_t) ((r[u] >> 8) & 0xffu);
				v[u][2] = (int8_t) ((r[u] >> 16) & 0xffu);
				v[u][3] = (int8_t) (r[u] >> 24);
			}
			break;
		}
		}
	}
}

// one normalised predicate on a widened value (sel_eval of select.hip with
// the mode under a wave-uniform branch)
__device__ __forceinline__ bool
ss_eval(const SsP &p, int64_t v)
{
	switch (p.mode) {
	case SEL_RANGE:
		return v >= p.vl && v <= p.vh;
	case SEL_ANTI:
		return p.nil_matches ? (v == p.nil || v <= p.vl || v >= p.vh) : (v != p.nil && (v <= p.vl || v >= p.vh));
	case SEL_EQ:
		return v == p.vl;
	case SEL_EQNIL:
		return v == p.nil;
	default:
		return v != p.nil;
	}
}

inline bool
aligned16(const void *p)
{
	return ((uintptr_t) p & 15) == 0;
}

// an in-scope column: 1, 2, 4 or 8 bytes on an integer base type
inline bool
ss_column(const mgdk_bat *b)
{
	if (b == nullptr)
		return false;
	switch (b->ttype) {
	case MGDK_bte: case MGDK_sht: case MGDK_int: case MGDK_lng:
	case MGDK_date: case MGDK_daytime: case MGDK_timestamp:
		break;
	default:
		return false;
	}
	return b->twidth == width_of(b->ttype) && (b->theap != nullptr || b->count == 0);
}

inline int64_t
ss_nil(int w)
{
	return w == 1 ? INT8_MIN : w == 2 ? INT16_MIN : w == 4 ? (int64_t) INT32_MIN : INT64_MIN;
}

// one predicate through BATselect's normalisation: the outcome, or -1 when
// the operators have to answer (an argument they reject).  tnonil: whether
// the values selected on are known to hold no nil -- the column's own
// property, except where they are gathered through a join index
template <typename T>
int
ss_normalise(const mgdk_selpred &p, SsP *o, bool tnonil)
{
	const void *tl = p.tl, *th = p.th;
	bool li = p.li, hi = p.hi, anti = p.anti, nil_matches = p.nil_matches;
	ThetaArgs ta;
	if (tl == nullptr)
		return -1;
	if (p.op) {
		const int rc = theta_args(basetype(p.b->ttype), tl, p.op, &ta);
		if (rc < 0)
			return -1;
		if (rc == 1)
			return SELN_EMPTY;
		tl = ta.tl, th = ta.th, li = ta.li, hi = ta.hi, anti = ta.anti, nil_matches = ta.nil_matches;
	}
	SelPred<T> sp{};
	const SelOutcome r = sel_normalise<T>(tnonil, (const T *) tl, (const T *) th, li, hi, anti, nil_matches, &sp);
	o->mode = sp.mode;
	o->nil_matches = sp.nil_matches;
	o->vl = (int64_t) sp.vl;
	o->vh = (int64_t) sp.vh;
	o->nil = (int64_t) Lim<T>::nil();
	return r;
}

template <typename T>
int
ss_normalise(const mgdk_selpred &p, SsP *o)
{
	return ss_normalise<T>(p, o, p.b->tnonil != 0);
}

// ss_normalise at the predicate column's width
inline int
ss_normalise_w(const mgdk_selpred &p, SsP *o, bool tnonil)
{
	switch (p.b->twidth) {
	case 1: return ss_normalise<int8_t>(p, o, tnonil);
	case 2: return ss_normalise<int16_t>(p, o, tnonil);
	case 4: return ss_normalise<int32_t>(p, o, tnonil);
	default: return ss_normalise<int64_t>(p, o, tnonil);
	}
}

inline int
ss_normalise_w(const mgdk_selpred &p, SsP *o)
{
	return ss_normalise_w(p, o, p.b->tnonil != 0);
}

}  // namespace
}  // namespace mgdk
