// selectgroupsum_hash.h -- the fragment of selectgroupsum.hip ("cascade of
// range / theta selects, GROUP BY, exact hge sums of a column or of a product
// of up to three (constant +- column) factors, and counts", one pass) for
// wider keys and more groups: one or two key columns of 1, 2, 4 or 8 bytes,
// together at most 8, and up to 256 groups (mgdk_select_groupsum_hash_fused,
// selectgroupsum_hash.hip), and the same with columns of a
// dimension table reached through a join index
// (mgdk_select_groupsum_star_fused, selectgroupsum_star.hip).
// The kernel and the entry are templates over the argument block: GhArgs is
// the hashed entry's, GhStarArgs adds the routes; the gather exists in the
// star instantiations only.
//
// The cascade is k_ss's (selectsum.h), as in k_gs: a wave owns 256-row
// chunks, lane l the rows 4l .. 4l+3, the first predicate's column is read
// whole and every later column only by lanes that hold a live row.  What
// differs from k_gs:
//
//   * a row's key code is k0 | k1 << 8 w0, each key masked to its width: one
//     64-bit word.  Its group slot is an entry of an open-addressing table of
//     512 entries in LDS: hash, read the entry, compare-and-swap only where
//     it was seen empty, next entry otherwise, at most 512 steps.  Every
//     64-bit value is a legal code, so the value that marks an empty entry
//     (all ones) has an entry of its own, number 512, outside the probed
//     range: a row with that code takes it without any swap.  An entry is
//     occupied when its count is not 0;
//   * count, first row and, per sum, low word, high word and nil count are
//     indexed by entry.  Where all live rows of a wave's batch have one slot
//     (sorted or clustered keys) the wave adds up in registers and one lane
//     adds to LDS; otherwise each row adds its own term (gs_add128);
//   * the minima and maxima of the tracked columns are reduced across the
//     wave in registers, then one LDS atomic per wave, column and batch;
//   * at its end a workgroup adds its occupied entries into one table in
//     global memory (the same addressing, device-scope atomics) that
//     k_gh_init prepared; k_gh_fin ranks the occupied entries by first row --
//     BATgroup's numbering -- and writes one result block.
//
// No loop here waits for a value that another lane writes: the probe loops
// are bounded by the table's size, and a full table raises `over`.
//
// A gathered use (star instantiations): the join index V, an oid column of
// the fact table, is loaded for the chunk like any 8-byte column -- by the
// lanes that hold a live row, whole under the first predicate -- and each
// live row's o - hseqbase(dimension) indexes one element of the dimension
// column, the loads of all rows of the batch issued before the first use.  A
// nil oid yields the dimension type's nil, as BATproject does; an oid outside
// the dimension, or a nil oid into a str key, on a live row raises `over`:
// the operators raise an error there, so they have to answer.  Dead rows load
// nothing and decide nothing.
#pragma once
#include <mutex>
#include <type_traits>

#include "selectgroupsum.h"

namespace mgdk {
namespace {

constexpr int GH_MAXG = 256;                 // groups of a result
constexpr int GH_ENT = 512;                  // probed entries (a power of two)
constexpr int GH_MARK = GH_ENT;              // the entry of the code that equals GH_EMPTY
constexpr int GH_SLOTS = GH_ENT + 1;
constexpr unsigned long long GH_EMPTY = ~0ull;
constexpr int GH_THREADS = 1024, GH_WAVES = GH_THREADS / 64;
#ifndef MGDK_GH_UNROLL
#define MGDK_GH_UNROLL 2
#endif
// chunks in flight per wave in the form that gathers: with two, the oids, the
// indexes and the gathered values of 8 rows do not fit the 128 VGPRs that 16
// waves per workgroup leave a lane
#ifndef MGDK_GH_STAR_UNROLL
#define MGDK_GH_STAR_UNROLL 1
#endif

struct GhK {
	const char *col;
	int w, count;             // count: first use of the column, its lines are counted here
	int shift, pad;
	uint64_t mask;
};
// the merged table; cell = entry * GS_MAXS + sum
struct GhGlob {
	unsigned long long code[GH_SLOTS], cnt[GH_SLOTS], first[GH_SLOTS];
	unsigned long long lo[GH_SLOTS * GS_MAXS], hi[GH_SLOTS * GS_MAXS], nil[GH_SLOTS * GS_MAXS];
	long long mn[GS_MAXT], mx[GS_MAXT];
	unsigned long long lines;
	uint32_t over, pad;
	unsigned long long gathers;
};
// the result block: groups ordered by first row
struct GhRes {
	uint32_t ng, over;
	unsigned long long lines;
	long long mn[GS_MAXT], mx[GS_MAXT];
	unsigned long long code[GH_MAXG], first[GH_MAXG], cnt[GH_MAXG];
	unsigned long long lo[GH_MAXG * GS_MAXS], hi[GH_MAXG * GS_MAXS], nil[GH_MAXG * GS_MAXS];
	unsigned long long gathers;
};
struct GhArgs {
	static constexpr bool star = false;
	SsP p[SS_MAXP];
	GhK k[GS_MAXK];
	GsS s[GS_MAXS];
	int np, nk, ns, nt;
	uint64_t c0, c1;          // chunks [c0, c1) of 256 rows
	uint64_t n;               // rows of the range
	GhGlob *glob;
};
// a route: the join index at the first row of the range and the extent of
// the dimension column it leads to
constexpr int GH_MAXV = 16;
struct GhVia {
	const char *via;
	uint64_t dseq;            // the dimension column's hseqbase
	uint32_t dcount;          // its rows, below 2^31
	int str;                  // a str key: a nil oid is refused (the device BATproject does)
};
// the star entry's block.  A use (predicate, key, factor) of a dimension
// column keeps that column's base and width in its `col` / `w` and names its
// route here: 0 a fact column; else 1 + the route, GH_VCOUNT set where the
// join index is used for the first time and its lines are counted
constexpr unsigned GH_VCOUNT = 0x80u;
struct GhStarArgs : GhArgs {
	static constexpr bool star = true;
	GhVia v[GH_MAXV];
	uint8_t rp[SS_MAXP], rk[GS_MAXK], rf[GS_MAXS][GS_MAXF];
};
// a workgroup's table in dynamic LDS, as offsets in 8-byte words: word 0 the
// `over` flag, word 1 the lines, then code / cnt / first [GH_SLOTS],
// lo / hi / nil [GH_SLOTS * ns] (cell = entry * ns + sum), mm [nt][2]
struct GhT {
	uint32_t code, cnt, first, lo, hi, nil, mm, words;
};
__host__ __device__ inline GhT
gh_layout(int ns, int nt)
{
	GhT t;
	t.code = 2;
	t.cnt = t.code + GH_SLOTS;
	t.first = t.cnt + GH_SLOTS;
	t.lo = t.first + GH_SLOTS;
	t.hi = t.lo + GH_SLOTS * ns;
	t.nil = t.hi + GH_SLOTS * ns;
	t.mm = t.nil + GH_SLOTS * ns;
	t.words = t.mm + 2 * nt;
	return t;
}

__device__ __forceinline__ uint32_t
gh_hash(unsigned long long code)
{
	// multiplicative, the top bits: codes that differ only in high bits
	// (i << 20, i << 32) or only in low bits spread alike
	code ^= code >> 32;
	return (uint32_t) ((code * 0x9e3779b97f4a7c15ull) >> 55);
}
static_assert(GH_ENT == 1 << (64 - 55), "gh_hash yields an entry number");

// the entry of `code` in the table `codes` (LDS or global): the marker's own
// entry, else the first probed entry that holds the code or that this lane
// could claim; -1: GH_ENT entries probed, the table is full
__device__ __forceinline__ int
gh_slot(unsigned long long *codes, unsigned long long code)
{
	if (code == GH_EMPTY)
		return GH_MARK;
	uint32_t e = gh_hash(code);
	for (int i = 0; i < GH_ENT; i++, e = (e + 1) & (GH_ENT - 1)) {
		unsigned long long c = __hip_atomic_load(&codes[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (c == GH_EMPTY)
			c = atomicCAS(&codes[e], GH_EMPTY, code);
		if (c == GH_EMPTY || c == code)
			return (int) e;
	}
	return -1;
}

// the second step of a gathered use: v holds the join index's oids of the
// batch, mb the live rows (bit 4u + k).  On return v holds the dimension
// column's values of the live rows, sign-extended: nil for a nil oid, and for
// an oid that no row of the dimension has (which raises the flag in L[0], as
// does a nil oid into a str key).  All 4 U loads are issued before the first
// is used; a dead row issues none.  gath: live rows with a non-nil oid
template <int U>
__device__ __forceinline__ void
gh_gather(const char *dim, int w, const GhVia &r, uint32_t mb, int64_t (&v)[U][4], unsigned long long *L,
	  uint32_t &gath)
{
	uint32_t idx[U][4], ok = 0, bad = 0, asked = 0;
#pragma unroll
	for (int u = 0; u < U; u++)
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const uint64_t o = (uint64_t) v[u][k], d = o - r.dseq;
			const uint32_t lv = mb >> (4 * u + k) & 1u;
			const bool isnil = o == MGDK_OID_NIL, in = d < (uint64_t) r.dcount;
			idx[u][k] = (uint32_t) d;
			asked |= (lv & (uint32_t) !isnil) << (4 * u + k);
			ok |= (lv & (uint32_t) (!isnil && in)) << (4 * u + k);
			bad |= (lv & (uint32_t) (isnil ? r.str != 0 : !in)) << (4 * u + k);
		}
	gath += (uint32_t) __popc(asked);
	if (bad)
		L[0] = 1;                        // the operators' error: they answer
	const int64_t nil = (int64_t) (~0ull << (8 * w - 1));   // the minimum of the width
	switch (w) {
	case 8: {
		int64_t x[U][4];
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				x[u][k] = ok >> (4 * u + k) & 1u ? ((const int64_t *) dim)[idx[u][k]] : nil;
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				v[u][k] = x[u][k];
		break;
	}
	case 4: {
		int32_t x[U][4];
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				x[u][k] = ok >> (4 * u + k) & 1u ? ((const int32_t *) dim)[idx[u][k]] : (int32_t) nil;
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				v[u][k] = x[u][k];
		break;
	}
	case 2: {
		int16_t x[U][4];
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				x[u][k] = ok >> (4 * u + k) & 1u ? ((const int16_t *) dim)[idx[u][k]] : (int16_t) nil;
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				v[u][k] = x[u][k];
		break;
	}
	default: {
		int8_t x[U][4];
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				x[u][k] = ok >> (4 * u + k) & 1u ? ((const int8_t *) dim)[idx[u][k]] : (int8_t) nil;
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				v[u][k] = x[u][k];
		break;
	}
	}
}

// one column of the batch into va: a fact column's rows, or (star) a
// dimension column's values through the use's route
template <int U, bool PLAIN, typename A>
__device__ __forceinline__ void
gh_column(const A &a, const char *col, int w, int count, unsigned route, const uint64_t (&ch)[U],
	  const uint32_t (&rows)[U], unsigned lane, uint32_t mb, bool (&live)[U], uint32_t &lines, uint32_t &gath,
	  int64_t (&va)[U][4], unsigned long long *L)
{
	bool viaed = false;
	if constexpr (A::star)
		viaed = route != 0;
	const int lw = viaed ? 8 : w;
	const bool cnt = viaed ? (route & GH_VCOUNT) != 0 : count != 0;
#pragma unroll
	for (int u = 0; u < U; u++) {
		live[u] = (mb >> (4 * u) & 15u) != 0;
		if (cnt)
			lines += ss_lines(lw, __ballot(live[u]));
	}
	if constexpr (A::star) {
		if (viaed) {
			const GhVia &r = a.v[(route & ~GH_VCOUNT) - 1];
			ss_load<U, PLAIN>(r.via, 8, ch, rows, lane, live, va);
			gh_gather<U>(col, w, r, mb, va, L, gath);
			return;
		}
	}
	ss_load<U, PLAIN>(col, w, ch, rows, lane, live, va);
}

// the cascade, the keys and the sums over U chunks, all loads of one column
// in flight together; valid[u] false: no such chunk (the odd one of a pair)
template <int U, bool PLAIN, typename A>
__device__ __forceinline__ void
gh_chunks(const A &a, const uint64_t (&ch)[U], const bool (&valid)[U], unsigned lane, uint32_t &lines,
	  uint32_t &gath, unsigned long long *L, const GhT &t)
{
	// the rows' liveness is a bit per row in a vector register (bit 4u + k)
	bool live[U];
	uint32_t rows[U], mb = 0;
	int64_t va[U][4];
#pragma unroll
	for (int u = 0; u < U; u++) {
		const uint64_t left = valid[u] ? a.n - ch[u] * 256 : 0;
		rows[u] = left < 256 ? (uint32_t) left : 256u;
#pragma unroll
		for (int k = 0; k < 4; k++)
			mb |= (uint32_t) (PLAIN ? 4 * lane + k < rows[u] : valid[u]) << (4 * u + k);
	}
	// rolled loops over the predicates, keys, sums and factors (one load
	// site each), as in k_ss
#pragma unroll 1
	for (int i = 0; i < a.np; i++) {
		const SsP &p = a.p[i];
		unsigned route = 0;
		if constexpr (A::star)
			route = a.rp[i];
		gh_column<U, PLAIN>(a, p.col, p.w, p.count, route, ch, rows, lane, mb, live, lines, gath, va, L);
		uint32_t pass = 0;
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				pass |= (uint32_t) ss_eval(p, va[u][k]) << (4 * u + k);
		mb &= pass;
	}
	if (__ballot(mb != 0) == 0)
		return;                          // no survivor in this wave's chunks
	unsigned long long code[U][4] = {};
#pragma unroll 1
	for (int j = 0; j < a.nk; j++) {
		const GhK &kc = a.k[j];
		unsigned route = 0;
		if constexpr (A::star)
			route = a.rk[j];
		gh_column<U, PLAIN>(a, kc.col, kc.w, kc.count, route, ch, rows, lane, mb, live, lines, gath, va, L);
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				code[u][k] |= ((unsigned long long) va[u][k] & kc.mask) << kc.shift;
	}
	// slots; a dead row has none
	int slot[U][4];
#pragma unroll
	for (int u = 0; u < U; u++)
#pragma unroll
		for (int k = 0; k < 4; k++) {
			int s = -1;
			if (mb >> (4 * u + k) & 1) {
				s = gh_slot(L + t.code, code[u][k]);
				if (s < 0) {
					L[0] = 1;            // more codes than entries
					mb &= ~(1u << (4 * u + k));
				}
			}
			slot[u][k] = s;
		}
	// do all live rows of the batch share one slot?
	int ls = -1;
	bool mixed = false;
#pragma unroll
	for (int u = 0; u < U; u++)
#pragma unroll
		for (int k = 0; k < 4; k++)
			if (slot[u][k] >= 0) {
				mixed = mixed || (ls >= 0 && slot[u][k] != ls);
				ls = ls < 0 ? slot[u][k] : ls;
			}
	const uint64_t hb = __ballot(ls >= 0);
	if (hb == 0)
		return;
	const int s0 = __shfl(ls, __ffsll((unsigned long long) hb) - 1);
	const bool uniform = __ballot(ls >= 0 && (mixed || ls != s0)) == 0;
	if (uniform) {
		// counts and first row from the ballots, one lane adds
		uint32_t cnt = 0;
		uint64_t first = ~0ull;
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const uint64_t b = __ballot(slot[u][k] >= 0);
				if (b != 0) {
					const uint64_t r = ch[u] * 256 + 4u * (uint32_t) (__ffsll((unsigned long long) b) - 1) + k;
					cnt += (uint32_t) __popcll(b);
					first = r < first ? r : first;
				}
			}
		if (lane == 0) {
			atomicAdd(&L[t.cnt + s0], (unsigned long long) cnt);
			if (first < __hip_atomic_load(&L[t.first + s0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
				atomicMin(&L[t.first + s0], (unsigned long long) first);
		}
	} else {
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				if (slot[u][k] >= 0) {
					const unsigned long long r = ch[u] * 256 + 4 * lane + k;
					atomicAdd(&L[t.cnt + slot[u][k]], 1ull);
					if (r < __hip_atomic_load(&L[t.first + slot[u][k]], __ATOMIC_RELAXED,
								  __HIP_MEMORY_SCOPE_WORKGROUP))
						atomicMin(&L[t.first + slot[u][k]], r);
				}
	}
#pragma unroll 1
	for (int j = 0; j < a.ns; j++) {
		const GsS &s = a.s[j];
		uhge term[U][4];
		uint32_t nilbits = 0;            // bit 4u + k: a factor of that row is nil
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				term[u][k] = 1;
#pragma unroll 1
		for (int q = 0; q < s.nf; q++) {
			const GsF &f = s.f[q];
			unsigned route = 0;
			if constexpr (A::star)
				route = a.rf[j][q];
			gh_column<U, PLAIN>(a, f.col, f.w, f.count, route, ch, rows, lane, mb, live, lines, gath, va, L);
#pragma unroll
			for (int u = 0; u < U; u++)
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const int64_t v = va[u][k];
					// wrapping: a factor that leaves lng is found by
					// the host from the minimum and maximum
					const uint64_t x = f.op == '+' ? (uint64_t) f.cst + (uint64_t) v
							 : f.op == '-' ? (uint64_t) f.cst - (uint64_t) v : (uint64_t) v;
					term[u][k] *= (uhge) (hge) (int64_t) x;
					nilbits |= (uint32_t) (v == f.nil) << (4 * u + k);
				}
			if (f.track) {
				// over the live non-nil rows only: a row the cascade
				// removed must not decide anything
				long long mn = INT64_MAX, mx = INT64_MIN;
#pragma unroll
				for (int u = 0; u < U; u++)
#pragma unroll
					for (int k = 0; k < 4; k++)
						if (slot[u][k] >= 0 && va[u][k] != f.nil) {
							mn = va[u][k] < mn ? va[u][k] : mn;
							mx = va[u][k] > mx ? va[u][k] : mx;
						}
#pragma unroll
				for (int o = 32; o > 0; o >>= 1) {
					const long long m2 = __shfl_xor(mn, o), x2 = __shfl_xor(mx, o);
					mn = m2 < mn ? m2 : mn;
					mx = x2 > mx ? x2 : mx;
				}
				if (lane == 0 && mn <= mx) {
					long long *w = (long long *) (L + t.mm) + 2 * (f.track - 1);
					__hip_atomic_fetch_min(&w[0], mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					__hip_atomic_fetch_max(&w[1], mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				}
			}
		}
		if (uniform) {
			// the lane's rows, then the wave, in registers; lane 0 adds
			uhge acc = 0;
			uint32_t nils = 0;
#pragma unroll
			for (int u = 0; u < U; u++)
#pragma unroll
				for (int k = 0; k < 4; k++)
					if (slot[u][k] >= 0) {
						if (!(nilbits >> (4 * u + k) & 1))
							acc += term[u][k];
						else
							nils++;
					}
			unsigned long long lo = (unsigned long long) acc, hi = (unsigned long long) (acc >> 64);
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) {
				const unsigned long long l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
				const uhge x = (((uhge) hi << 64) | lo) + (((uhge) h2 << 64) | l2);
				lo = (unsigned long long) x;
				hi = (unsigned long long) (x >> 64);
				nils += __shfl_xor(nils, o);
			}
			if (lane == 0) {
				const int cell = s0 * a.ns + j;
				if (lo | hi)
					gs_add128(&L[t.lo + cell], &L[t.hi + cell], lo, hi);
				if (nils)
					atomicAdd(&L[t.nil + cell], (unsigned long long) nils);
			}
		} else {
#pragma unroll
			for (int u = 0; u < U; u++)
#pragma unroll
				for (int k = 0; k < 4; k++)
					if (slot[u][k] >= 0) {
						const int cell = slot[u][k] * a.ns + j;
						if (!(nilbits >> (4 * u + k) & 1))
							gs_add128(&L[t.lo + cell], &L[t.hi + cell], (unsigned long long) term[u][k],
								  (unsigned long long) (term[u][k] >> 64));
						else
							atomicAdd(&L[t.nil + cell], 1ull);
					}
		}
	}
}

__global__ __launch_bounds__(256) void
k_gh_init(GhGlob *g)
{
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < GH_SLOTS * GS_MAXS; i += gridDim.x * blockDim.x) {
		g->lo[i] = 0;
		g->hi[i] = 0;
		g->nil[i] = 0;
		if (i < GH_SLOTS) {
			g->code[i] = GH_EMPTY;
			g->cnt[i] = 0;
			g->first[i] = ~0ull;
		}
		if (i < GS_MAXT) {
			g->mn[i] = INT64_MAX;
			g->mx[i] = INT64_MIN;
		}
		if (i == 0) {
			g->lines = 0;
			g->over = 0;
			g->gathers = 0;
		}
	}
}

// A: GhArgs, or GhStarArgs for the form that gathers (one word of LDS more,
// after the table: the gathers)
template <int U, bool PLAIN, typename A>
__global__ __launch_bounds__(GH_THREADS) void
k_gh(A a)
{
	extern __shared__ unsigned long long gh_lds[];
	unsigned long long *L = gh_lds;
	const GhT t = gh_layout(a.ns, a.nt);
	for (unsigned i = threadIdx.x; i < t.words; i += GH_THREADS) {
		unsigned long long v = 0;
		if (i >= t.code && i < t.cnt)
			v = GH_EMPTY;
		else if (i >= t.first && i < t.lo)
			v = ~0ull;
		else if (i >= t.mm)
			v = (i - t.mm) & 1 ? (unsigned long long) INT64_MIN : (unsigned long long) INT64_MAX;
		L[i] = v;
	}
	if constexpr (A::star)
		if (threadIdx.x == 0)
			L[t.words] = 0;
	__syncthreads();
	uint32_t lines = 0, gath = 0;
	const unsigned lane = __lane_id();
	const uint64_t nw = (uint64_t) gridDim.x * GH_WAVES;
	// the wave's chunk index, told to the compiler as wave-uniform: the
	// buffer descriptors built from it then live in scalar registers
	uint64_t c = a.c0 + (uint64_t) blockIdx.x * GH_WAVES +
		     (unsigned) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
	for (; c < a.c1; c += U * nw) {
		uint64_t ch[U];
		bool valid[U];
#pragma unroll
		for (int u = 0; u < U; u++) {
			ch[u] = c + u * nw;
			valid[u] = ch[u] < a.c1;
		}
		gh_chunks<U, PLAIN>(a, ch, valid, lane, lines, gath, L, t);
	}
	// the line count is per wave (from ballots): lane 0 carries it
	if (lane == 0 && lines)
		atomicAdd(&L[1], (unsigned long long) lines);
	if constexpr (A::star) {
		// the gathers are per lane
#pragma unroll
		for (int o = 32; o > 0; o >>= 1)
			gath += __shfl_xor(gath, o);
		if (lane == 0 && gath)
			atomicAdd(&L[t.words], (unsigned long long) gath);
	}
	__syncthreads();
	// the workgroup's occupied entries into the global table
	GhGlob *g = a.glob;
	for (unsigned e = threadIdx.x; e < GH_SLOTS; e += GH_THREADS) {
		const unsigned long long cnt = L[t.cnt + e];
		if (cnt == 0)
			continue;
		const int ge = gh_slot(g->code, e == GH_MARK ? GH_EMPTY : L[t.code + e]);
		if (ge < 0) {
			g->over = 1;
			continue;
		}
		atomicAdd(&g->cnt[ge], cnt);
		if (L[t.first + e] < __hip_atomic_load(&g->first[ge], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
			atomicMin(&g->first[ge], L[t.first + e]);
		for (int j = 0; j < a.ns; j++) {
			const unsigned long long lo = L[t.lo + e * a.ns + j], hi = L[t.hi + e * a.ns + j];
			const unsigned long long nl = L[t.nil + e * a.ns + j];
			if (lo | hi)
				gs_add128(&g->lo[ge * GS_MAXS + j], &g->hi[ge * GS_MAXS + j], lo, hi);
			if (nl)
				atomicAdd(&g->nil[ge * GS_MAXS + j], nl);
		}
	}
	if ((int) threadIdx.x < a.nt) {
		const long long *w = (const long long *) (L + t.mm) + 2 * threadIdx.x;
		if (w[0] <= w[1]) {
			__hip_atomic_fetch_min(&g->mn[threadIdx.x], w[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			__hip_atomic_fetch_max(&g->mx[threadIdx.x], w[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
	if (threadIdx.x == GH_THREADS - 1) {
		if (L[1])
			atomicAdd(&g->lines, L[1]);
		if (L[0])
			g->over = 1;
		if constexpr (A::star)
			if (L[t.words])
				atomicAdd(&g->gathers, L[t.words]);
	}
}

// the occupied entries of the merged table ranked by first row (BATgroup
// numbers the groups by first occurrence) into the result block
__global__ __launch_bounds__(GH_THREADS) void
k_gh_fin(const GhGlob *g, int ns, int nt, GhRes *out)
{
	__shared__ unsigned long long sfirst[GH_SLOTS];
	__shared__ uint32_t sng;
	const unsigned e = threadIdx.x;
	const bool occ = e < GH_SLOTS && g->cnt[e] != 0;
	if (e < GH_SLOTS)
		sfirst[e] = occ ? g->first[e] : ~0ull;
	if (e == 0)
		sng = 0;
	__syncthreads();
	if (occ)
		atomicAdd(&sng, 1u);
	__syncthreads();
	const uint32_t ng = sng;
	if (e == 0) {
		out->ng = ng;
		out->over = g->over;
		out->lines = g->lines;
		out->gathers = g->gathers;
	}
	if ((int) e < nt) {
		out->mn[e] = g->mn[e];
		out->mx[e] = g->mx[e];
	}
	if (!occ || ng > GH_MAXG)
		return;
	// first rows are distinct: the rank is the number of smaller ones
	const unsigned long long mine = sfirst[e];
	uint32_t rank = 0;
	for (int i = 0; i < GH_SLOTS; i++)
		rank += sfirst[i] < mine;
	out->code[rank] = e == GH_MARK ? GH_EMPTY : g->code[e];
	out->first[rank] = mine;
	out->cnt[rank] = g->cnt[e];
	for (int j = 0; j < ns; j++) {
		out->lo[rank * GS_MAXS + j] = g->lo[e * GS_MAXS + j];
		out->hi[rank * GS_MAXS + j] = g->hi[e * GS_MAXS + j];
		out->nil[rank * GS_MAXS + j] = g->nil[e * GS_MAXS + j];
	}
}

// a key column: what ss_column takes, or str offsets of 1 or 2 bytes into a
// heap small enough that equal strings share an offset (BATgroup's own
// condition for grouping on the offsets, group.hip)
inline bool
gh_key(const mgdk_bat *b, bool *isstr)
{
	*isstr = false;
	if (ss_column(b))
		return true;
	if (b == nullptr || b->ttype != MGDK_str || (b->twidth != 1 && b->twidth != 2) ||
	    (b->theap == nullptr && b->count != 0))
		return false;
	*isstr = true;
	return b->tvheap != nullptr && b->tvheapsize < ((uint64_t) 1 << 16);
}

// the entry of both forms.  STAR: a column whose descriptor is some
// vias[i].col is a dimension column reached through vias[i].via; every other
// column, and every via, is of the fact table.  Without STAR vias is not read
template <bool STAR>
inline int
gh_entry(const mgdk_selpred *preds, int npreds, mgdk_bat *s, mgdk_bat *const *keys, int nkeys,
	 const mgdk_gsumexpr *sums, int nsums, const mgdk_starvia *vias, int nvias, int maxgroups, int *ngroups,
	 mgdk_gsgroupw *groups, void *sumres, uint64_t *nonnil, unsigned long long *last_lines,
	 unsigned long long *last_gathers)
{
	using A = std::conditional_t<STAR, GhStarArgs, GhArgs>;
	constexpr int UN = STAR ? MGDK_GH_STAR_UNROLL : MGDK_GH_UNROLL;
	if (npreds < 0 || npreds > SS_MAXP || (npreds > 0 && preds == nullptr) || keys == nullptr || nkeys < 1 ||
	    nkeys > GS_MAXK || nsums < 0 || nsums > GS_MAXS || ngroups == nullptr || groups == nullptr || maxgroups < 0 ||
	    (nsums > 0 && (sums == nullptr || sumres == nullptr || nonnil == nullptr)))
		return 1;
	if (!STAR)
		nvias = 0;
	if (nvias < 0 || nvias > GH_MAXV || (nvias > 0 && vias == nullptr))
		return 1;
	for (int i = 0; i < nvias; i++) {
		const mgdk_bat *v = vias[i].via, *d = vias[i].col;
		if (v == nullptr || d == nullptr || v->ttype != MGDK_oid || v->twidth != 8 ||
		    (v->theap == nullptr && v->count != 0) || d->count >= ((uint64_t) 1 << 31))
			return 1;
	}
	// the route of a column: 1 + its index in vias, 0 for a fact column
	auto route = [&](const mgdk_bat *b) {
		for (int i = 0; i < nvias; i++)
			if (vias[i].col == b)
				return i + 1;
		return 0;
	};
	auto via_of = [&](const mgdk_bat *b) -> const mgdk_bat * {
		const int r = route(b);
		return r ? vias[r - 1].via : nullptr;
	};
	const mgdk_bat *b0 = npreds > 0 ? preds[0].b : keys[0];
	if (b0 == nullptr)
		return 1;
	if (via_of(b0))
		b0 = via_of(b0);
	// of the fact table: the column itself, or the join index that leads to it
	auto same = [&](const mgdk_bat *b) {
		const mgdk_bat *v = via_of(b);
		if (v)
			b = v;
		return b->count == b0->count && b->hseqbase == b0->hseqbase;
	};
	for (int i = 0; i < nvias; i++)
		if (vias[i].via->count != b0->count || vias[i].via->hseqbase != b0->hseqbase)
			return 1;
	for (int i = 0; i < npreds; i++)
		if (!ss_column(preds[i].b) || !same(preds[i].b))
			return 1;
	bool kstr[GS_MAXK] = {};
	int kbytes = 0;
	for (int j = 0; j < nkeys; j++) {
		if (!gh_key(keys[j], &kstr[j]) || !same(keys[j]))
			return 1;
		kbytes += keys[j]->twidth;
	}
	if (kbytes > 8)
		return 1;                        // a row's key code is one 64-bit word
	if (!gs_sums_ok(sums, nsums, same))
		return 1;
	if (s && (s->ttype != MGDK_void || is_complex_cand(s) || s->tseqbase == MGDK_OID_NIL))
		return 1;
	// the predicates, normalised: an argument the operators reject leaves
	// the whole request to them; "all candidates" drops the predicate
	A a{};
	bool empty = false;
	const void *seen[SS_MAXP + GS_MAXK + GS_MAXT + GH_MAXV];
	int nseen = 0;
	auto first_heap = [&](const void *heap) {
		for (int k = 0; k < nseen; k++)
			if (seen[k] == heap)
				return 0;
		seen[nseen++] = heap;
		return 1;
	};
	// a dimension column's own lines are not counted (its gathers are); its
	// join index counts as an 8-byte column at its first use
	auto first_use = [&](const mgdk_bat *b) { return via_of(b) ? 0 : first_heap(b->theap); };
	auto via_use = [&](const mgdk_bat *b, bool counted) {
		const int r = route(b);
		if (r == 0)
			return 0u;
		return (unsigned) r | (first_heap(vias[r - 1].via->theap) && counted ? GH_VCOUNT : 0u);
	};
	bool gathered_before = false;
	for (int i = 0; i < npreds; i++) {
		SsP p{};
		// the values a gathered predicate selects on hold a nil wherever the
		// join index holds a nil oid, whatever the dimension column knows
		// about itself
		const bool viaed = via_of(preds[i].b) != nullptr;
		const int r = viaed ? ss_normalise_w(preds[i], &p, false) : ss_normalise_w(preds[i], &p);
		if (r < 0)
			return 1;
		// the operators project before they select: where a gathered
		// predicate is decided without a scan, or no row is left after
		// one, an oid that they would refuse goes unseen here
		if ((viaed && r != SELN_SCAN) || (r == SELN_EMPTY && gathered_before))
			return 1;
		gathered_before = gathered_before || viaed;
		if (r == SELN_EMPTY)
			empty = true;
		if (r != SELN_SCAN)
			continue;
		p.w = preds[i].b->twidth;
		p.col = (const char *) preds[i].b->theap;
		// the first predicate's column is read whole and not counted
		p.count = first_use(preds[i].b) && a.np > 0;
		if constexpr (STAR)
			a.rp[a.np] = (uint8_t) via_use(preds[i].b, a.np > 0);
		a.p[a.np++] = p;
	}
	Cand ci;
	if (cand_init(&ci, b0, s) < 0)
		return -1;
	*last_lines = 0;
	*last_gathers = 0;
	*ngroups = 0;
	if (empty || ci.n == 0)
		return 0;
	const uint64_t first = ci.seq - b0->hseqbase;
	a.n = ci.n;
	a.nk = nkeys;
	a.ns = nsums;
	bool al = true;
	for (int i = 0; i < a.np; i++) {
		if constexpr (STAR)
			if (a.rp[i])
				continue;                // a dimension column starts at its own first row
		a.p[i].col += first * (uint64_t) a.p[i].w;
		al = al && aligned16(a.p[i].col);
	}
	for (int j = 0; j < nkeys; j++) {
		GhK &k = a.k[j];
		const bool dim = via_of(keys[j]) != nullptr;
		k.w = keys[j]->twidth;
		k.col = (const char *) keys[j]->theap + (dim ? 0 : first * (uint64_t) k.w);
		k.count = first_use(keys[j]);
		k.shift = j == 0 ? 0 : 8 * a.k[0].w;
		k.mask = k.w == 8 ? ~(uint64_t) 0 : ((uint64_t) 1 << (8 * k.w)) - 1;
		al = al && (dim || aligned16(k.col));
		if constexpr (STAR)
			a.rk[j] = (uint8_t) via_use(keys[j], true);
	}
	// which sums need their columns' minima and maxima: the shared rule
	GsTrack tr;
	gs_plan_sums(sums, nsums, a.n, first, a.s, tr, al, first_use, via_of);
	a.nt = tr.nt;
	if constexpr (STAR) {
		for (int j = 0; j < nsums; j++)
			for (int q = 0; q < sums[j].nf; q++)
				a.rf[j][q] = (uint8_t) via_use(sums[j].f[q].b, true);
		for (int i = 0; i < nvias; i++) {
			GhVia &v = a.v[i];
			v.via = (const char *) vias[i].via->theap + first * 8;
			v.dseq = vias[i].col->hseqbase;
			v.dcount = (uint32_t) vias[i].col->count;
			v.str = vias[i].col->ttype == MGDK_str;
			al = al && aligned16(v.via);
		}
	}
	// one workgroup of 16 waves per CU of 256 CUs: its table takes up to
	// 87 KB of the CU's 160 KiB of LDS; 2 chunks in flight per wave
	constexpr unsigned MAXWG = 256u;
	const uint64_t nfull = al ? a.n / 256 : 0, nall = (a.n + 255) / 256;
	const unsigned g1 = nfull ? grid_for(nfull, GH_WAVES * UN, MAXWG) : 0;
	const unsigned g2 = nall > nfull ? grid_for(nall - nfull, GH_WAVES, MAXWG) : 0;
	char *dev = (char *) scratch(sizeof(GhGlob) + sizeof(GhRes));
	GhRes *h = (GhRes *) pinned(sizeof(GhRes));
	if (dev == nullptr || h == nullptr)
		return -1;
	GhGlob *glob = (GhGlob *) dev;
	GhRes *out = (GhRes *) (dev + sizeof(GhGlob));
	const size_t lds = ((size_t) gh_layout(a.ns, a.nt).words + (STAR ? 1 : 0)) * 8;
	// beyond the default limit of dynamic LDS from two sums on.  The limit
	// belongs to the kernel, not to the calling thread: it only ever grows,
	// under a lock, so no thread lowers what another one's launch needs
	static std::mutex lds_mu;
	static size_t lds_set = 0;
	{
		std::lock_guard<std::mutex> lds_lock(lds_mu);
		if (lds > lds_set) {
			if (!hip_ok(hipFuncSetAttribute((const void *) k_gh<UN, false, A>,
							hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds), "LDS size") ||
			    !hip_ok(hipFuncSetAttribute((const void *) k_gh<1, true, A>,
							hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds), "LDS size"))
				return -1;
			lds_set = lds;
		}
	}
	hipStream_t st = stream();
	a.glob = glob;
	{
		ProfScope prof(STAR ? "select_groupsum_star_fused" : "select_groupsum_hash_fused");
		hipLaunchKernelGGL(k_gh_init, dim3(13), dim3(256), 0, st, glob);
		if (g1) {
			a.c0 = 0;
			a.c1 = nfull;
			hipLaunchKernelGGL((k_gh<UN, false, A>), dim3(g1), dim3(GH_THREADS), lds, st, a);
		}
		if (g2) {
			a.c0 = nfull;
			a.c1 = nall;
			hipLaunchKernelGGL((k_gh<1, true, A>), dim3(g2), dim3(GH_THREADS), lds, st, a);
		}
		hipLaunchKernelGGL(k_gh_fin, dim3(1), dim3(GH_THREADS), 0, st, glob, a.ns, a.nt, out);
	}
	if (!hip_ok(hipMemcpyAsync(h, out, sizeof(GhRes), hipMemcpyDeviceToHost, st), "memcpy") || !sync())
		return -1;
	if (h->over || h->ng > GH_MAXG || (int) h->ng > maxgroups)
		return 1;
	uint64_t total = 0;
	for (uint32_t g = 0; g < h->ng; g++)
		total += h->cnt[g];
	if (!gs_sums_exact(sums, nsums, total, tr, h->mn, h->mx, via_of))
		return 1;
	for (uint32_t g = 0; g < h->ng; g++) {
		mgdk_gsgroupw &o = groups[g];
		memset(&o, 0, sizeof(o));
		o.first = ci.seq + h->first[g];
		o.count = h->cnt[g];
		for (int j = 0; j < nkeys; j++) {
			const uint64_t v = (h->code[g] >> a.k[j].shift) & a.k[j].mask;
			const int sh = 64 - 8 * a.k[j].w;
			// the tail value sign-extended; a str key's offset is unsigned
			o.key[j] = kstr[j] ? (int64_t) v : (int64_t) (v << sh) >> sh;
		}
		for (int j = 0; j < nsums; j++) {
			const int cell = (int) g * GS_MAXS + j;
			const uint64_t nn = h->cnt[g] - h->nil[cell];
			const hge v = nn ? (hge) (((uhge) h->hi[cell] << 64) | h->lo[cell]) : Lim<hge>::nil();
			memcpy((char *) sumres + 16 * ((size_t) g * nsums + j), &v, 16);
			nonnil[(size_t) g * nsums + j] = nn;
		}
	}
	*ngroups = (int) h->ng;
	*last_lines = h->lines;
	*last_gathers = h->gathers;
	return 0;
}

}  // namespace
}  // namespace mgdk
