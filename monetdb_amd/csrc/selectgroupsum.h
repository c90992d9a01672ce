// selectgroupsum.h -- what the two fused select-cascade GROUP BY kernels share
// (selectgroupsum.hip: one-byte keys, 8 groups; selectgroupsum_hash.h: keys
// of up to 8 bytes together, 256 groups): the sum / factor descriptions, the
// 128-bit add, and the host-side overflow rule -- which columns need their
// minimum and maximum kept, and the final check of the factors' ranges and of
// survivors x the product of the largest magnitudes.  One rule for both
// entries.  DESIGN.md 11.11, 11.12.
#pragma once
#include "selectsum.h"

namespace mgdk {
namespace {

constexpr int GS_MAXK = 2, GS_MAXS = 6, GS_MAXF = 3;
constexpr int GS_MAXT = GS_MAXS * GS_MAXF;   // columns whose minimum / maximum can be wanted

struct GsF {
	const char *col;          // the column at the first row of the range
	int w, op;                // op 0: col; '+': cst + col; '-': cst - col
	int count;                // first use of the column: its lines are counted here
	int track;                // 1 + its minimum / maximum slot, at the column's first use; else 0
	int64_t nil, cst;
};
struct GsS {
	GsF f[GS_MAXF];
	int nf, pad;
};
// the columns whose minimum and maximum over the live non-nil rows are kept.
// A column reached through a join index (selectgroupsum_hash.h) is the pair
// of both heaps -- the values its live rows gather -- and via is NULL for a
// column of the table itself
struct GsTrack {
	const void *col[GS_MAXT], *via[GS_MAXT];
	int w[GS_MAXT];
	int nt;
};

// cell += (hi, lo) modulo 2^128: a returning add on the low word tells this
// lane the carry its own add produced, whatever else was added meanwhile
__device__ __forceinline__ void
gs_add128(unsigned long long *lo, unsigned long long *hi, unsigned long long tlo, unsigned long long thi)
{
	const unsigned long long old = atomicAdd(lo, tlo);
	thi += old + tlo < old;
	if (thi)
		atomicAdd(hi, thi);
}

inline uhge
gs_mag(hge v)
{
	return v < 0 ? (uhge) 0 - (uhge) v : (uhge) v;
}

constexpr uhge GS_LIM = ((uhge) 1 << 127) - 1;

inline uhge
gs_sat_mul(uhge x, uhge y)
{
	return (x != 0 && y > GS_LIM / x) ? GS_LIM + 1 : x * y;
}

// the request's shape, checked the same way by both entries: every sum has
// one to three factors, each an in-scope column of the common count and
// hseqbase, alone or as cst +- column
template <typename Same>
inline bool
gs_sums_ok(const mgdk_gsumexpr *sums, int nsums, Same same)
{
	for (int j = 0; j < nsums; j++) {
		if (sums[j].nf < 1 || sums[j].nf > GS_MAXF)
			return false;
		for (int q = 0; q < sums[j].nf; q++) {
			const mgdk_gsfactor &f = sums[j].f[q];
			if (!ss_column(f.b) || !same(f.b) || (f.op != 0 && f.op != '+' && f.op != '-') ||
			    (f.op != 0 && f.cst == INT64_MIN))
				return false;
		}
	}
	return true;
}

// the sums for the kernel.  A column's values lie within its type's width:
// where that bounds every factor within lng and rows x the product of the
// factors' magnitudes below 2^127, the sum needs no minima and maxima;
// otherwise each of its columns is tracked (at its first such use).  `al`
// is cleared when an operand does not start 16-byte aligned.  via_of(b): the
// join index through which b is reached, NULL for a column of the table; such
// a b starts at its own first row and need not be aligned.
template <typename FirstUse, typename ViaOf>
inline void
gs_plan_sums(const mgdk_gsumexpr *sums, int nsums, uint64_t rows, uint64_t first, GsS *out, GsTrack &tr, bool &al,
	     FirstUse first_use, ViaOf via_of)
{
	constexpr uhge lng_max = (uhge) INT64_MAX;
	tr.nt = 0;
	for (int j = 0; j < nsums; j++) {
		GsS &x = out[j];
		x.nf = sums[j].nf;
		uhge bound = rows;
		bool want = false;
		for (int q = 0; q < x.nf; q++) {
			const mgdk_gsfactor &f = sums[j].f[q];
			const uhge mw = ((uhge) 1 << (8 * f.b->twidth - 1)) - 1;
			const uhge mf = f.op ? gs_mag((hge) f.cst) + mw : mw;
			if (mf > lng_max)
				want = true;
			bound = gs_sat_mul(bound, mf);
		}
		want = want || bound > GS_LIM;
		for (int q = 0; q < x.nf; q++) {
			const mgdk_gsfactor &f = sums[j].f[q];
			GsF &o = x.f[q];
			const mgdk_bat *via = via_of(f.b);
			const void *vh = via ? via->theap : nullptr;
			o.w = f.b->twidth;
			o.col = (const char *) f.b->theap + (via ? 0 : first * (uint64_t) o.w);
			o.op = f.op;
			o.cst = f.cst;
			o.nil = ss_nil(o.w);
			o.count = first_use(f.b);
			al = al && (via || aligned16(o.col));
			if (want) {
				int k = 0;
				while (k < tr.nt && (tr.col[k] != f.b->theap || tr.via[k] != vh))
					k++;
				if (k == tr.nt) {
					tr.col[tr.nt] = f.b->theap;
					tr.via[tr.nt] = vh;
					tr.w[tr.nt++] = o.w;
					o.track = k + 1;     // the kernel keeps them at this use only
				}
			}
		}
	}
}

inline const mgdk_bat *
gs_no_via(const mgdk_bat *)
{
	return nullptr;
}

template <typename FirstUse>
inline void
gs_plan_sums(const mgdk_gsumexpr *sums, int nsums, uint64_t rows, uint64_t first, GsS *out, GsTrack &tr, bool &al,
	     FirstUse first_use)
{
	gs_plan_sums(sums, nsums, rows, first, out, tr, al, first_use, gs_no_via);
}

// every factor's range from the survivors' minimum and maximum (the type's
// width where they were not kept): outside lng the operators raise, or a
// value would be taken for nil.  Then B = survivors x the product of the
// factors' largest magnitudes >= the sum of |term| in any order, every
// intermediate product included: below 2^127 nothing can overflow and the
// wrapped sums are the true ones.  false: the operators have to answer
template <typename ViaOf>
inline bool
gs_sums_exact(const mgdk_gsumexpr *sums, int nsums, uint64_t survivors, const GsTrack &tr, const long long *mns,
	      const long long *mxs, ViaOf via_of)
{
	for (int j = 0; j < nsums; j++) {
		uhge bound = survivors;
		for (int q = 0; q < sums[j].nf; q++) {
			const mgdk_gsfactor &f = sums[j].f[q];
			hge mn = -(hge) (((uhge) 1 << (8 * f.b->twidth - 1)) - 1), mx = -mn;
			const mgdk_bat *via = via_of(f.b);
			const void *vh = via ? via->theap : nullptr;
			for (int k = 0; k < tr.nt; k++)
				if (tr.col[k] == f.b->theap && tr.via[k] == vh) {
					mn = mns[k];
					mx = mxs[k];
				}
			if (mn > mx) {               // no live non-nil value: no term
				bound = 0;
				continue;
			}
			hge lo = mn, hi = mx;
			if (f.op == '+')
				lo = (hge) f.cst + mn, hi = (hge) f.cst + mx;
			else if (f.op == '-')
				lo = (hge) f.cst - mx, hi = (hge) f.cst - mn;
			if (f.op && (lo < -(hge) INT64_MAX || hi > (hge) INT64_MAX))
				return false;
			const uhge ml = gs_mag(lo), mh = gs_mag(hi);
			bound = gs_sat_mul(bound, ml > mh ? ml : mh);
		}
		if (bound > GS_LIM)
			return false;
	}
	return true;
}

inline bool
gs_sums_exact(const mgdk_gsumexpr *sums, int nsums, uint64_t survivors, const GsTrack &tr, const long long *mns,
	      const long long *mxs)
{
	return gs_sums_exact(sums, nsums, survivors, tr, mns, mxs, gs_no_via);
}

}  // namespace
}  // namespace mgdk
