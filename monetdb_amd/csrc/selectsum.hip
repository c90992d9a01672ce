// selectsum.hip -- the plan fragment "cascade of range / theta selects over
// aligned integer columns, then exact sums of a column or of a product of two
// columns over the survivors" in one pass (mgdk_select_sum_fused; DESIGN.md
// 11.10).  TPC-H Q6 is one instance; mgdk_q6_fused (tpch.hip) stays the
// hand-tuned special case.
//
// Host side: every predicate goes through BATselect's own normalisation
// (selnorm.h), which answers "empty", "all candidates" or one closed
// predicate {mode, vl, vh, nil_matches}; the kernel sees only the last kind,
// with the bounds and the nil widened to int64.
//
// Device side (k_ss): a wave owns 256-row chunks, lane l the rows 4l .. 4l+3
// of its chunk, so a column of width w is one load of 4w bytes per lane (two
// 16-byte loads for w = 8), chosen by a wave-uniform switch on w.  The first
// predicate's column is read for every row; every later column -- predicate
// or operand -- only by lanes that still hold a live row: a dead lane passes
// an out-of-range offset to a raw buffer load whose descriptor covers just
// the chunk, and the range check answers zeros without touching memory.  A
// 128-byte line of a later column is therefore fetched only when one of its
// rows survived everything before it.  Sums are accumulated modulo 2^128 per
// lane, reduced per workgroup into one partial, and added up by k_ss_fin:
// integers, so any order gives the same bits.
//
// The last, partial chunk -- and every chunk of columns whose heap is not
// 16-byte aligned (BATslice views, a dense candidate starting mid-column) --
// runs the same cascade with plain per-row loads guarded by the row count
// (k_ss<1, true>), so no lane reads past a heap.
#include "selectsum.h"

using namespace mgdk;

namespace {

constexpr int SS_MAXS = 4;
// launch shape of the main kernel: chunks in flight per wave, workgroups per CU
#ifndef MGDK_SS_UNROLL
#define MGDK_SS_UNROLL 2
#endif
#ifndef MGDK_SS_BPC
#define MGDK_SS_BPC 8
#endif

struct SsS {
	const char *a, *b;        // b NULL: sum(a)
	int wa, wb, ca, cb;       // widths; first use of a / b (line count)
	int wantmax, pad;         // the product can reach 2^127: keep max|a|, max|b|
	int64_t nila, nilb;
};
struct SsPart {
	unsigned long long lo[SS_MAXS], hi[SS_MAXS];    // the sums, modulo 2^128
	unsigned long long nn[SS_MAXS];                 // non-nil terms
	unsigned long long ma[SS_MAXS], mb[SS_MAXS];    // max|a|, max|b| over those terms
	unsigned long long cnt, lines;
};
struct SsArgs {
	SsP p[SS_MAXP];
	SsS s[SS_MAXS];
	int np, ns;
	uint64_t c0, c1;          // chunks [c0, c1) of 256 rows
	uint64_t n;               // rows of the range
	SsPart *parts;            // one per workgroup
};
struct SsAcc {
	hge sum[SS_MAXS];
	uint32_t nn[SS_MAXS];
	unsigned long long ma[SS_MAXS], mb[SS_MAXS];
	uint32_t cnt, lines;
};

__device__ __forceinline__ unsigned long long
ss_abs(int64_t v)
{
	return v < 0 ? 0ull - (unsigned long long) v : (unsigned long long) v;
}

// the cascade and the sums over U chunks, all loads of one column in flight
// together; valid[u] false: no such chunk (the odd one out of a pair)
template <int U, bool PLAIN>
__device__ __forceinline__ void
ss_chunks(const SsArgs &a, const uint64_t (&ch)[U], const bool (&valid)[U], unsigned lane, SsAcc &acc)
{
	bool m[U][4], live[U];
	uint32_t rows[U];
	int64_t va[U][4], vb[U][4];
#pragma unroll
	for (int u = 0; u < U; u++) {
		const uint64_t left = valid[u] ? a.n - ch[u] * 256 : 0;
		rows[u] = left < 256 ? (uint32_t) left : 256u;
#pragma unroll
		for (int k = 0; k < 4; k++)
			m[u][k] = PLAIN ? 4 * lane + k < rows[u] : valid[u];
	}
	auto lanes = [&](bool count, int w) {
#pragma unroll
		for (int u = 0; u < U; u++) {
			live[u] = m[u][0] || m[u][1] || m[u][2] || m[u][3];
			if (count)
				acc.lines += ss_lines(w, __ballot(live[u]));
		}
	};
	// rolled loops over the predicates and the sums (one load site each for a
	// predicate, a first and a second operand): the descriptors come from
	// the kernel arguments by a wave-uniform index
#pragma unroll 1
	for (int i = 0; i < a.np; i++) {
		const SsP &p = a.p[i];
		lanes(p.count != 0, p.w);
		ss_load<U, PLAIN>(p.col, p.w, ch, rows, lane, live, va);
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				m[u][k] = m[u][k] && ss_eval(p, va[u][k]);
	}
#pragma unroll
	for (int u = 0; u < U; u++)
#pragma unroll
		for (int k = 0; k < 4; k++)
			acc.cnt += m[u][k];
#pragma unroll 1
	for (int j = 0; j < a.ns; j++) {
		const SsS &s = a.s[j];
		hge t = 0;
		uint32_t nn = 0;
		unsigned long long ma = 0, mb = 0;
		lanes(s.ca != 0, s.wa);
		ss_load<U, PLAIN>(s.a, s.wa, ch, rows, lane, live, va);
		if (s.b != nullptr) {
			lanes(s.cb != 0, s.wb);
			ss_load<U, PLAIN>(s.b, s.wb, ch, rows, lane, live, vb);
#pragma unroll
			for (int u = 0; u < U; u++)
#pragma unroll
				for (int k = 0; k < 4; k++)
					if (m[u][k] && va[u][k] != s.nila && vb[u][k] != s.nilb) {
						t += (hge) va[u][k] * (hge) vb[u][k];
						nn++;
						if (s.wantmax) {
							const unsigned long long x = ss_abs(va[u][k]), y = ss_abs(vb[u][k]);
							ma = x > ma ? x : ma;
							mb = y > mb ? y : mb;
						}
					}
		} else {
#pragma unroll
			for (int u = 0; u < U; u++)
#pragma unroll
				for (int k = 0; k < 4; k++)
					if (m[u][k] && va[u][k] != s.nila) {
						t += (hge) va[u][k];
						nn++;
					}
		}
		// into the sum's own registers (wave-uniform compare, no indexing)
#pragma unroll
		for (int q = 0; q < SS_MAXS; q++)
			if (q == j) {
				acc.sum[q] += t;
				acc.nn[q] += nn;
				acc.ma[q] = ma > acc.ma[q] ? ma : acc.ma[q];
				acc.mb[q] = mb > acc.mb[q] ? mb : acc.mb[q];
			}
	}
}

// one partial per workgroup from every thread's values (blockDim.x == 256)
__device__ __forceinline__ void
ss_publish(int ns, const hge (&sum)[SS_MAXS], const unsigned long long (&nn)[SS_MAXS],
	   const unsigned long long (&ma)[SS_MAXS], const unsigned long long (&mb)[SS_MAXS], unsigned long long cnt,
	   unsigned long long lines, SsPart *out)
{
	auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
	auto mx = [](unsigned long long x, unsigned long long y) { return x > y ? x : y; };
	SsPart pt{};
#pragma unroll
	for (int j = 0; j < SS_MAXS; j++) {
		if (j < ns) {
			const hge t = block_sum128(sum[j]);
			pt.lo[j] = (unsigned long long) (uhge) t;
			pt.hi[j] = (unsigned long long) ((uhge) t >> 64);
			pt.nn[j] = block_reduce(nn[j], add);
			pt.ma[j] = block_reduce(ma[j], mx);
			pt.mb[j] = block_reduce(mb[j], mx);
		}
	}
	pt.cnt = block_reduce(cnt, add);
	pt.lines = block_reduce(lines, add);
	if (threadIdx.x == 0)
		*out = pt;
}

template <int U, bool PLAIN>
__global__ __launch_bounds__(256) void
k_ss(SsArgs a)
{
	SsAcc acc{};
	const unsigned lane = __lane_id();
	const uint64_t nw = (uint64_t) gridDim.x * 4;
	// the wave's chunk index, told to the compiler as wave-uniform: the
	// buffer descriptors built from it then live in scalar registers
	uint64_t c = a.c0 + (uint64_t) blockIdx.x * 4 + (unsigned) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
	for (; c < a.c1; c += U * nw) {
		uint64_t ch[U];
		bool valid[U];
#pragma unroll
		for (int u = 0; u < U; u++) {
			ch[u] = c + u * nw;
			valid[u] = ch[u] < a.c1;
		}
		ss_chunks<U, PLAIN>(a, ch, valid, lane, acc);
	}
	unsigned long long nn[SS_MAXS];
#pragma unroll
	for (int j = 0; j < SS_MAXS; j++)
		nn[j] = acc.nn[j];
	// the line count is per wave (from ballots): lane 0 carries it
	ss_publish(a.ns, acc.sum, nn, acc.ma, acc.mb, acc.cnt, lane == 0 ? acc.lines : 0, a.parts + blockIdx.x);
}

// *out = the partials added up (the maxima: their maximum)
__global__ __launch_bounds__(256) void
k_ss_fin(const SsPart *parts, uint32_t n, int ns, SsPart *out)
{
	hge sum[SS_MAXS] = {};
	unsigned long long nn[SS_MAXS] = {}, ma[SS_MAXS] = {}, mb[SS_MAXS] = {}, cnt = 0, lines = 0;
	for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
		const SsPart *p = parts + i;
#pragma unroll
		for (int j = 0; j < SS_MAXS; j++) {
			if (j < ns) {
				sum[j] += (hge) (((uhge) p->hi[j] << 64) | p->lo[j]);
				nn[j] += p->nn[j];
				ma[j] = p->ma[j] > ma[j] ? p->ma[j] : ma[j];
				mb[j] = p->mb[j] > mb[j] ? p->mb[j] : mb[j];
			}
		}
		cnt += p->cnt;
		lines += p->lines;
	}
	ss_publish(ns, sum, nn, ma, mb, cnt, lines, out);
}

thread_local unsigned long long ss_last_lines = 0;

}  // namespace

extern "C" {

int
mgdk_select_sum_fused(const mgdk_selpred *preds, int npreds, mgdk_bat *s, const mgdk_sumexpr *sums, int nsums,
		      void *results, uint64_t *count)
{
	if (preds == nullptr || npreds < 1 || npreds > SS_MAXP || nsums < 0 || nsums > SS_MAXS ||
	    (nsums > 0 && (sums == nullptr || results == nullptr)))
		return 1;
	const mgdk_bat *b0 = preds[0].b;
	auto in_scope = [b0](const mgdk_bat *b) {
		return ss_column(b) && b->count == b0->count && b->hseqbase == b0->hseqbase;
	};
	if (b0 == nullptr)
		return 1;
	for (int i = 0; i < npreds; i++)
		if (!in_scope(preds[i].b))
			return 1;
	for (int j = 0; j < nsums; j++)
		if (!in_scope(sums[j].a) || (sums[j].b && !in_scope(sums[j].b)))
			return 1;
	if (s && (s->ttype != MGDK_void || is_complex_cand(s) || s->tseqbase == MGDK_OID_NIL))
		return 1;
	// the predicates, normalised: an argument the operators reject leaves
	// the whole request to them; "all candidates" drops the predicate
	SsArgs a{};
	bool empty = false;
	const mgdk_bat *seen[SS_MAXP + 2 * SS_MAXS];
	int nseen = 0;
	auto first_use = [&](const mgdk_bat *b) {
		for (int k = 0; k < nseen; k++)
			if (seen[k]->theap == b->theap)
				return 0;
		seen[nseen++] = b;
		return 1;
	};
	for (int i = 0; i < npreds; i++) {
		SsP p{};
		int r;
		switch (preds[i].b->twidth) {
		case 1: r = ss_normalise<int8_t>(preds[i], &p); break;
		case 2: r = ss_normalise<int16_t>(preds[i], &p); break;
		case 4: r = ss_normalise<int32_t>(preds[i], &p); break;
		default: r = ss_normalise<int64_t>(preds[i], &p); break;
		}
		if (r < 0)
			return 1;
		if (r == SELN_EMPTY)
			empty = true;
		if (r != SELN_SCAN)
			continue;
		p.w = preds[i].b->twidth;
		p.col = (const char *) preds[i].b->theap;
		// the first predicate's column is read whole and not counted
		p.count = first_use(preds[i].b) && a.np > 0;
		a.p[a.np++] = p;
	}
	Cand ci;
	if (cand_init(&ci, b0, s) < 0)
		return -1;
	hge *res = (hge *) results;
	auto put = [res](int j, hge v) { memcpy((char *) res + 16 * (size_t) j, &v, 16); };
	ss_last_lines = 0;
	if (empty || ci.n == 0) {
		for (int j = 0; j < nsums; j++)
			put(j, Lim<hge>::nil());
		if (count)
			*count = 0;
		return 0;
	}
	const uint64_t first = ci.seq - b0->hseqbase;
	a.n = ci.n;
	a.ns = nsums;
	bool al = true;
#pragma unroll 1
	for (int i = 0; i < a.np; i++) {
		a.p[i].col += first * (uint64_t) a.p[i].w;
		al = al && aligned16(a.p[i].col);
	}
	for (int j = 0; j < nsums; j++) {
		SsS &x = a.s[j];
		const mgdk_bat *ba = sums[j].a, *bb = sums[j].b;
		x.wa = ba->twidth;
		x.a = (const char *) ba->theap + first * (uint64_t) x.wa;
		x.nila = ss_nil(x.wa);
		x.ca = first_use(ba);
		al = al && aligned16(x.a);
		if (bb) {
			x.wb = bb->twidth;
			x.b = (const char *) bb->theap + first * (uint64_t) x.wb;
			x.nilb = ss_nil(x.wb);
			x.cb = first_use(bb);
			// |a * b| <= 2^(8 (wa + wb) - 2) and n < 2^k rows: the terms
			// cannot add up to 2^127 while k + 8 (wa + wb) - 2 <= 127 --
			// always for operands of 8 bytes or less together, below 2^33
			// rows for 12 bytes -- and such a sum skips the maxima
			x.wantmax = (64 - __builtin_clzll(a.n)) + 8 * (x.wa + x.wb) - 2 > 127;
			al = al && aligned16(x.b);
		}
	}
	// launch shape: 2 chunks in flight per wave and at most 8 workgroups per
	// CU of 256 CUs -- Q6 over 60M rows ran 0.35 ms at 4, 8 or 16 workgroups
	// per CU, 0.46 at 64 and 0.54 at 128 (a workgroup ends in ~20 block
	// reductions and one 176-byte partial); 4 chunks in flight cost half the
	// occupancy and ran 0.47 ms
	constexpr unsigned MAXG = 256u * MGDK_SS_BPC;
	const uint64_t nfull = al ? a.n / 256 : 0, nall = (a.n + 255) / 256;
	const unsigned g1 = nfull ? grid_for(nfull, 4 * MGDK_SS_UNROLL, MAXG) : 0;
	const unsigned g2 = nall > nfull ? grid_for(nall - nfull, 4, MAXG) : 0;
	SsPart *parts = (SsPart *) scratch((size_t) (g1 + g2) * sizeof(SsPart));
	SsPart *out = (SsPart *) meta_buf();
	SsPart *h = (SsPart *) pinned(sizeof(SsPart));
	if (parts == nullptr || out == nullptr || h == nullptr)
		return -1;
	hipStream_t st = stream();
	{
		ProfScope prof("select_sum_fused");
		if (g1) {
			a.c0 = 0;
			a.c1 = nfull;
			a.parts = parts;
			hipLaunchKernelGGL((k_ss<MGDK_SS_UNROLL, false>), dim3(g1), dim3(256), 0, st, a);
		}
		if (g2) {
			a.c0 = nfull;
			a.c1 = nall;
			a.parts = parts + g1;
			hipLaunchKernelGGL((k_ss<1, true>), dim3(g2), dim3(256), 0, st, a);
		}
		hipLaunchKernelGGL(k_ss_fin, dim3(1), dim3(256), 0, st, parts, g1 + g2, a.ns, out);
	}
	if (!hip_ok(hipMemcpyAsync(h, out, sizeof(SsPart), hipMemcpyDeviceToHost, st), "memcpy") || !sync())
		return -1;
	// B = terms x max|a| x max|b| >= the sum of |term| in any order: below
	// 2^127 no prefix can overflow and the wrapped sum is the true one;
	// otherwise the operators decide by the reference's running-sum rule
	const uhge lim = ((uhge) 1 << 127) - 1;
	for (int j = 0; j < nsums; j++) {
		if (!a.s[j].wantmax)
			continue;
		const uhge mm = (uhge) h->ma[j] * (uhge) h->mb[j];
		if (mm != 0 && (uhge) h->nn[j] > lim / mm)
			return 1;
	}
	for (int j = 0; j < nsums; j++)
		put(j, h->nn[j] ? (hge) (((uhge) h->hi[j] << 64) | h->lo[j]) : Lim<hge>::nil());
	if (count)
		*count = h->cnt;
	ss_last_lines = h->lines;
	return 0;
}

unsigned long long
mgdk_select_sum_last_lines(void)
{
	return ss_last_lines;
}

}  // extern "C"
