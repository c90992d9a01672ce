// selectgroupsum.hip -- the plan fragment "cascade of range / theta selects,
// GROUP BY one or two one-byte keys, exact hge sums of a column or of a
// product of up to three (constant +- column) factors, and counts" in one
// pass (mgdk_select_groupsum_fused).  TPC-H Q1 is one
// instance; mgdk_q1_fused (tpch.hip) stays the hand-tuned special case.
//
// The cascade is k_ss's (selectsum.h): a wave owns 256-row chunks, lane l the
// rows 4l .. 4l+3, the first predicate's column is read whole and every
// later column -- predicate, key or operand -- only by lanes that hold a live
// row.  On top of it (k_gs):
//
//   * a row's key code is k0 | k1 << 8; its group slot is the code's place in
//     a table of 8 codes in LDS, filled on first sight by a compare-and-swap.
//     The wave reads the table once per batch into registers, so the swap
//     runs only for a code the table did not hold yet.  A ninth code raises
//     a flag and the host answers "not applicable";
//   * counts and first rows come from ballots per slot, one LDS atomic per
//     slot, batch and wave;
//   * a live non-nil term is added to its (slot, sum) cell in LDS with a
//     returning 64-bit add on the low word; the observed carry and the high
//     word go to the high word.  Each cell has 8 replicas chosen by lane so
//     that a wave's adds spread over 8 addresses.  Integers modulo 2^128, so
//     any order gives the same bits.  Nil terms are counted instead;
//   * for the columns whose type width does not already bound the result, each
//     thread keeps the minimum and maximum of the live non-nil values in LDS
//     words of its own (no atomics); the host decides from them whether a
//     factor can leave lng or a sum could overflow hge.
//
// A workgroup writes one table (GsPart); k_gs_fin merges the tables by code
// through the same LDS structure, orders the groups by first row -- BATgroup's
// numbering -- and writes one block that the host copies back with one wait.
#include "selectgroupsum.h"

using namespace mgdk;

namespace {

constexpr int GS_MAXG = 8;
constexpr int GS_CELLS = GS_MAXG * GS_MAXS;
constexpr int GS_REP = 8;                    // replicas of a sum cell
constexpr uint32_t GS_EMPTY = 0xffffffffu;   // no key code has more than 16 bits
#ifndef MGDK_GS_UNROLL
#define MGDK_GS_UNROLL 2
#endif
#ifndef MGDK_GS_BPC
#define MGDK_GS_BPC 8
#endif

struct GsK {
	const char *col;
	int count, pad;
};
// one workgroup's groups (slots in the order it met them); also the result
// block (groups ordered by first row)
struct GsPart {
	uint32_t code[GS_MAXG];
	unsigned long long first[GS_MAXG], cnt[GS_MAXG];
	unsigned long long lo[GS_CELLS], hi[GS_CELLS], nil[GS_CELLS];   // cell = slot * GS_MAXS + sum
	long long mn[GS_MAXT], mx[GS_MAXT];
	unsigned long long lines;
	uint32_t over, ng;
};
static_assert(sizeof(GsPart) <= 4096, "the result block goes through meta_buf()");
struct GsArgs {
	SsP p[SS_MAXP];
	GsK k[GS_MAXK];
	GsS s[GS_MAXS];
	int np, nk, ns, nt;
	uint64_t c0, c1;          // chunks [c0, c1) of 256 rows
	uint64_t n;               // rows of the range
	GsPart *parts;            // one per workgroup
};
struct GsTab {
	uint32_t code[GS_MAXG];
	uint32_t over, pad;
	unsigned long long first[GS_MAXG], cnt[GS_MAXG];
	unsigned long long nil[GS_CELLS];
	unsigned long long lo[GS_CELLS][GS_REP], hi[GS_CELLS][GS_REP];
};

__device__ __forceinline__ void
gs_tab_init(GsTab &t)
{
	for (unsigned i = threadIdx.x; i < GS_CELLS * GS_REP; i += blockDim.x) {
		(&t.lo[0][0])[i] = 0;
		(&t.hi[0][0])[i] = 0;
	}
	if (threadIdx.x < GS_CELLS)
		t.nil[threadIdx.x] = 0;
	if (threadIdx.x < GS_MAXG) {
		t.code[threadIdx.x] = GS_EMPTY;
		t.first[threadIdx.x] = ~0ull;
		t.cnt[threadIdx.x] = 0;
	}
	if (threadIdx.x == 0)
		t.over = 0;
}

// the slot of a code the caller did not find in its copy of the table: the
// first slot that holds it or that this lane could claim; -1: a ninth code
__device__ __forceinline__ int
gs_slot_claim(uint32_t *codes, uint32_t code)
{
	for (int g = 0; g < GS_MAXG; g++) {
		const uint32_t old = atomicCAS(&codes[g], GS_EMPTY, code);
		if (old == GS_EMPTY || old == code)
			return g;
	}
	return -1;
}

// replicas of a cell added up
__device__ __forceinline__ uhge
gs_fold(const GsTab &t, int cell)
{
	uhge s = 0;
	for (int r = 0; r < GS_REP; r++)
		s += ((uhge) t.hi[cell][r] << 64) | t.lo[cell][r];
	return s;
}

// the cascade, the keys and the sums over U chunks, all loads of one column
// in flight together; valid[u] false: no such chunk (the odd one of a pair)
template <int U, bool PLAIN>
__device__ __forceinline__ void
gs_chunks(const GsArgs &a, const uint64_t (&ch)[U], const bool (&valid)[U], unsigned lane, uint32_t &lines,
	  GsTab &t, long long *mm)
{
	// the rows' liveness is a bit per row in a vector register (bit 4u + k):
	// eight lane masks would cost sixteen scalar registers
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
	auto lanesb = [&](bool count, int w) {
#pragma unroll
		for (int u = 0; u < U; u++) {
			live[u] = (mb >> (4 * u) & 15u) != 0;
			if (count)
				lines += ss_lines(w, __ballot(live[u]));
		}
	};
	// rolled loops over the predicates, keys, sums and factors (one load
	// site each), as in k_ss: unrolled they spill
#pragma unroll 1
	for (int i = 0; i < a.np; i++) {
		const SsP &p = a.p[i];
		lanesb(p.count != 0, p.w);
		ss_load<U, PLAIN>(p.col, p.w, ch, rows, lane, live, va);
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
	uint32_t code[U][4] = {};
#pragma unroll 1
	for (int j = 0; j < a.nk; j++) {
		lanesb(a.k[j].count != 0, 1);
		ss_load<U, PLAIN>(a.k[j].col, 1, ch, rows, lane, live, va);
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				code[u][k] |= ((uint32_t) va[u][k] & 0xffu) << (8 * j);
	}
	// slots: against the table as it stands (one read for the wave), and by
	// compare-and-swap for the codes it does not hold yet
	int slot[U][4];
	bool miss = false;
	{
		uint32_t tc[GS_MAXG];
#pragma unroll
		for (int g = 0; g < GS_MAXG; g++)
			tc[g] = __hip_atomic_load(&t.code[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++) {
				int s = -1;
#pragma unroll
				for (int g = 0; g < GS_MAXG; g++)
					s = tc[g] == code[u][k] ? g : s;
				slot[u][k] = s;
				miss = miss || ((mb >> (4 * u + k) & 1) && s < 0);
			}
	}
	if (__ballot(miss) != 0) {
		// slot by slot for all rows (gs_slot_claim's walk, turned inside
		// out: one rolled loop, no loop under a row's branch)
#pragma unroll 1
		for (int g = 0; g < GS_MAXG; g++)
#pragma unroll
			for (int u = 0; u < U; u++)
#pragma unroll
				for (int k = 0; k < 4; k++)
					if ((mb >> (4 * u + k) & 1) && slot[u][k] < 0) {
						const uint32_t old = atomicCAS(&t.code[g], GS_EMPTY, code[u][k]);
						if (old == GS_EMPTY || old == code[u][k])
							slot[u][k] = g;
					}
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				if ((mb >> (4 * u + k) & 1) && slot[u][k] < 0) {
					t.over = 1;              // a ninth code
					mb &= ~(1u << (4 * u + k));
				}
	}
	// a dead row has no slot: the tests below are on the slot alone
#pragma unroll
	for (int u = 0; u < U; u++)
#pragma unroll
		for (int k = 0; k < 4; k++)
			slot[u][k] = (mb >> (4 * u + k) & 1) ? slot[u][k] : -1;
	// counts and first rows: per slot, the ballots of its rows
#pragma unroll 1
	for (int g = 0; g < GS_MAXG; g++) {
		uint32_t cnt = 0;
		uint64_t first = ~0ull;
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const uint64_t b = __ballot(slot[u][k] == g);
				if (b != 0) {
					const uint64_t r = ch[u] * 256 + 4u * (uint32_t) (__ffsll((unsigned long long) b) - 1) + k;
					cnt += (uint32_t) __popcll(b);
					first = r < first ? r : first;
				}
			}
		if (cnt != 0 && lane == 0) {
			atomicAdd(&t.cnt[g], (unsigned long long) cnt);
			atomicMin(&t.first[g], (unsigned long long) first);
		}
	}
	const unsigned rep = lane & (GS_REP - 1);
#pragma unroll 1
	for (int j = 0; j < a.ns; j++) {
		const GsS &s = a.s[j];
		uhge term[U][4];
		uint32_t nilbits = 0;            // bit 4u + k: a factor of that row is nil (a lane mask per row costs scalar registers)
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				term[u][k] = 1;
#pragma unroll 1
		for (int q = 0; q < s.nf; q++) {
			const GsF &f = s.f[q];
			lanesb(f.count != 0, f.w);
			ss_load<U, PLAIN>(f.col, f.w, ch, rows, lane, live, va);
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
				long long *w = mm + ((size_t) (f.track - 1) * blockDim.x + threadIdx.x) * 2;
				if (mn < w[0])
					w[0] = mn;
				if (mx > w[1])
					w[1] = mx;
			}
		}
#pragma unroll
		for (int u = 0; u < U; u++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				if (slot[u][k] >= 0) {
					const int cell = slot[u][k] * GS_MAXS + j;
					if (!(nilbits >> (4 * u + k) & 1))
						gs_add128(&t.lo[cell][rep], &t.hi[cell][rep], (unsigned long long) term[u][k],
							  (unsigned long long) (term[u][k] >> 64));
					else
						atomicAdd(&t.nil[cell], 1ull);
				}
	}
}

// the workgroup's table, or the merged one, into *out; slots in table order
__device__ __forceinline__ void
gs_publish(const GsTab &t, GsPart *out)
{
	if (threadIdx.x < GS_CELLS) {
		const uhge s = gs_fold(t, threadIdx.x);
		out->lo[threadIdx.x] = (unsigned long long) s;
		out->hi[threadIdx.x] = (unsigned long long) (s >> 64);
		out->nil[threadIdx.x] = t.nil[threadIdx.x];
	}
	if (threadIdx.x < GS_MAXG) {
		out->code[threadIdx.x] = t.code[threadIdx.x];
		out->first[threadIdx.x] = t.first[threadIdx.x];
		out->cnt[threadIdx.x] = t.cnt[threadIdx.x];
	}
}

template <int U, bool PLAIN>
__global__ __launch_bounds__(256) void
k_gs(GsArgs a)
{
	extern __shared__ long long gs_mm[];     // [nt][256][2]: each thread's minima and maxima
	__shared__ GsTab t;
	gs_tab_init(t);
	for (int i = 0; i < a.nt; i++) {
		gs_mm[((size_t) i * 256 + threadIdx.x) * 2] = INT64_MAX;
		gs_mm[((size_t) i * 256 + threadIdx.x) * 2 + 1] = INT64_MIN;
	}
	__syncthreads();
	uint32_t lines = 0;
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
		gs_chunks<U, PLAIN>(a, ch, valid, lane, lines, t, gs_mm);
	}
	__syncthreads();
	GsPart *out = a.parts + blockIdx.x;
	gs_publish(t, out);
	auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
	auto mnf = [](long long x, long long y) { return x < y ? x : y; };
	auto mxf = [](long long x, long long y) { return x > y ? x : y; };
	// the line count is per wave (from ballots): lane 0 carries it
	const unsigned long long ln = block_reduce((unsigned long long) (lane == 0 ? lines : 0), add);
	if (threadIdx.x == 0) {
		out->lines = ln;
		out->over = t.over;
		out->ng = 0;
	}
	for (int i = 0; i < a.nt; i++) {
		const long long mn = block_reduce(gs_mm[((size_t) i * 256 + threadIdx.x) * 2], mnf);
		const long long mx = block_reduce(gs_mm[((size_t) i * 256 + threadIdx.x) * 2 + 1], mxf);
		if (threadIdx.x == 0) {
			out->mn[i] = mn;
			out->mx[i] = mx;
		}
	}
}

// the workgroups' tables merged by code, groups ordered by first row
__global__ __launch_bounds__(256) void
k_gs_fin(const GsPart *parts, uint32_t n, int ns, int nt, GsPart *out)
{
	__shared__ GsTab t;
	__shared__ GsPart res;
	gs_tab_init(t);
	__syncthreads();
	const unsigned rep = threadIdx.x & (GS_REP - 1);
	unsigned long long lines = 0;
	for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
		const GsPart *p = parts + i;
		lines += p->lines;
		if (p->over)
			t.over = 1;
		for (int g = 0; g < GS_MAXG; g++) {
			if (p->code[g] == GS_EMPTY)
				break;
			const int mg = gs_slot_claim(t.code, p->code[g]);
			if (mg < 0) {
				t.over = 1;
				continue;
			}
			atomicAdd(&t.cnt[mg], p->cnt[g]);
			atomicMin(&t.first[mg], p->first[g]);
			for (int j = 0; j < ns; j++) {
				gs_add128(&t.lo[mg * GS_MAXS + j][rep], &t.hi[mg * GS_MAXS + j][rep], p->lo[g * GS_MAXS + j],
					  p->hi[g * GS_MAXS + j]);
				if (p->nil[g * GS_MAXS + j])
					atomicAdd(&t.nil[mg * GS_MAXS + j], p->nil[g * GS_MAXS + j]);
			}
		}
	}
	__syncthreads();
	gs_publish(t, &res);
	auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
	auto mnf = [](long long x, long long y) { return x < y ? x : y; };
	auto mxf = [](long long x, long long y) { return x > y ? x : y; };
	lines = block_reduce(lines, add);
	if (threadIdx.x == 0)
		out->lines = lines;
	for (int s = 0; s < nt; s++) {
		long long mn = INT64_MAX, mx = INT64_MIN;
		for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
			mn = mnf(mn, parts[i].mn[s]);
			mx = mxf(mx, parts[i].mx[s]);
		}
		mn = block_reduce(mn, mnf);
		mx = block_reduce(mx, mxf);
		if (threadIdx.x == 0) {
			out->mn[s] = mn;
			out->mx[s] = mx;
		}
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		// BATgroup numbers the groups by first occurrence
		int ord[GS_MAXG], ng = 0;
		for (int g = 0; g < GS_MAXG; g++) {
			if (res.code[g] == GS_EMPTY)
				continue;
			int k = ng++;
			for (; k > 0 && res.first[ord[k - 1]] > res.first[g]; k--)
				ord[k] = ord[k - 1];
			ord[k] = g;
		}
		for (int i = 0; i < ng; i++) {
			const int g = ord[i];
			out->code[i] = res.code[g];
			out->first[i] = res.first[g];
			out->cnt[i] = res.cnt[g];
			for (int j = 0; j < GS_MAXS; j++) {
				out->lo[i * GS_MAXS + j] = res.lo[g * GS_MAXS + j];
				out->hi[i * GS_MAXS + j] = res.hi[g * GS_MAXS + j];
				out->nil[i * GS_MAXS + j] = res.nil[g * GS_MAXS + j];
			}
		}
		out->ng = (uint32_t) ng;
		out->over = t.over;
	}
}

thread_local unsigned long long gs_last_lines = 0;

// a key column: one byte per row -- bte, or str offsets into a heap small
// enough that equal strings share an offset (BATgroup's own condition for
// grouping on the offsets, group.hip)
bool
gs_key(const mgdk_bat *b)
{
	if (b == nullptr || b->twidth != 1 || (b->theap == nullptr && b->count != 0))
		return false;
	if (b->ttype == MGDK_bte)
		return true;
	return b->ttype == MGDK_str && b->tvheap != nullptr && b->tvheapsize < ((uint64_t) 1 << 16);
}

}  // namespace

extern "C" {

int
mgdk_select_groupsum_fused(const mgdk_selpred *preds, int npreds, mgdk_bat *s, mgdk_bat *const *keys, int nkeys,
			   const mgdk_gsumexpr *sums, int nsums, int maxgroups, int *ngroups, mgdk_gsgroup *groups,
			   void *sumres, uint64_t *nonnil)
{
	if (npreds < 0 || npreds > SS_MAXP || (npreds > 0 && preds == nullptr) || keys == nullptr || nkeys < 1 ||
	    nkeys > GS_MAXK || nsums < 0 || nsums > GS_MAXS || ngroups == nullptr || groups == nullptr || maxgroups < 0 ||
	    (nsums > 0 && (sums == nullptr || sumres == nullptr || nonnil == nullptr)))
		return 1;
	const mgdk_bat *b0 = npreds > 0 ? preds[0].b : keys[0];
	if (b0 == nullptr)
		return 1;
	auto same = [b0](const mgdk_bat *b) { return b->count == b0->count && b->hseqbase == b0->hseqbase; };
	for (int i = 0; i < npreds; i++)
		if (!ss_column(preds[i].b) || !same(preds[i].b))
			return 1;
	for (int j = 0; j < nkeys; j++)
		if (!gs_key(keys[j]) || !same(keys[j]))
			return 1;
	if (!gs_sums_ok(sums, nsums, same))
		return 1;
	if (s && (s->ttype != MGDK_void || is_complex_cand(s) || s->tseqbase == MGDK_OID_NIL))
		return 1;
	// the predicates, normalised: an argument the operators reject leaves
	// the whole request to them; "all candidates" drops the predicate
	GsArgs a{};
	bool empty = false;
	const void *seen[SS_MAXP + GS_MAXK + GS_MAXT];
	int nseen = 0;
	auto first_use = [&](const mgdk_bat *b) {
		for (int k = 0; k < nseen; k++)
			if (seen[k] == b->theap)
				return 0;
		seen[nseen++] = b->theap;
		return 1;
	};
	for (int i = 0; i < npreds; i++) {
		SsP p{};
		const int r = ss_normalise_w(preds[i], &p);
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
	gs_last_lines = 0;
	*ngroups = 0;
	if (empty || ci.n == 0)
		return 0;
	const uint64_t first = ci.seq - b0->hseqbase;
	a.n = ci.n;
	a.nk = nkeys;
	a.ns = nsums;
	bool al = true;
	for (int i = 0; i < a.np; i++) {
		a.p[i].col += first * (uint64_t) a.p[i].w;
		al = al && aligned16(a.p[i].col);
	}
	for (int j = 0; j < nkeys; j++) {
		a.k[j].col = (const char *) keys[j]->theap + first;
		a.k[j].count = first_use(keys[j]);
		al = al && aligned16(a.k[j].col);
	}
	// which sums need their columns' minima and maxima: the shared rule
	GsTrack tr;
	gs_plan_sums(sums, nsums, a.n, first, a.s, tr, al, first_use);
	a.nt = tr.nt;
	// launch shape as k_ss's: 2 chunks in flight per wave, at most 8
	// workgroups per CU of 256 CUs
	constexpr unsigned MAXG = 256u * MGDK_GS_BPC;
	const uint64_t nfull = al ? a.n / 256 : 0, nall = (a.n + 255) / 256;
	const unsigned g1 = nfull ? grid_for(nfull, 4 * MGDK_GS_UNROLL, MAXG) : 0;
	const unsigned g2 = nall > nfull ? grid_for(nall - nfull, 4, MAXG) : 0;
	GsPart *parts = (GsPart *) scratch((size_t) (g1 + g2) * sizeof(GsPart));
	GsPart *out = (GsPart *) meta_buf();
	GsPart *h = (GsPart *) pinned(sizeof(GsPart));
	if (parts == nullptr || out == nullptr || h == nullptr)
		return -1;
	const size_t lds = (size_t) a.nt * 256 * 2 * sizeof(long long);
	if (lds > 32768) {
		// beyond the default limit of dynamic LDS only for ten or more
		// tracked columns
		if (!hip_ok(hipFuncSetAttribute((const void *) k_gs<MGDK_GS_UNROLL, false>,
						hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds), "LDS size") ||
		    !hip_ok(hipFuncSetAttribute((const void *) k_gs<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
						(int) lds), "LDS size"))
			return -1;
	}
	hipStream_t st = stream();
	{
		ProfScope prof("select_groupsum_fused");
		if (g1) {
			a.c0 = 0;
			a.c1 = nfull;
			a.parts = parts;
			hipLaunchKernelGGL((k_gs<MGDK_GS_UNROLL, false>), dim3(g1), dim3(256), lds, st, a);
		}
		if (g2) {
			a.c0 = nfull;
			a.c1 = nall;
			a.parts = parts + g1;
			hipLaunchKernelGGL((k_gs<1, true>), dim3(g2), dim3(256), lds, st, a);
		}
		hipLaunchKernelGGL(k_gs_fin, dim3(1), dim3(256), 0, st, parts, g1 + g2, a.ns, a.nt, out);
	}
	if (!hip_ok(hipMemcpyAsync(h, out, sizeof(GsPart), hipMemcpyDeviceToHost, st), "memcpy") || !sync())
		return -1;
	if (h->over || h->ng > GS_MAXG || (int) h->ng > maxgroups)
		return 1;
	uint64_t total = 0;
	for (uint32_t g = 0; g < h->ng; g++)
		total += h->cnt[g];
	if (!gs_sums_exact(sums, nsums, total, tr, h->mn, h->mx))
		return 1;
	for (uint32_t g = 0; g < h->ng; g++) {
		mgdk_gsgroup &o = groups[g];
		memset(&o, 0, sizeof(o));
		o.first = ci.seq + h->first[g];
		o.count = h->cnt[g];
		o.key[0] = (uint8_t) (h->code[g] & 0xffu);
		o.key[1] = (uint8_t) (h->code[g] >> 8);
		for (int j = 0; j < nsums; j++) {
			const int cell = (int) g * GS_MAXS + j;
			const uint64_t nn = h->cnt[g] - h->nil[cell];
			const hge v = nn ? (hge) (((uhge) h->hi[cell] << 64) | h->lo[cell]) : Lim<hge>::nil();
			memcpy((char *) sumres + 16 * ((size_t) g * nsums + j), &v, 16);
			nonnil[(size_t) g * nsums + j] = nn;
		}
	}
	*ngroups = (int) h->ng;
	gs_last_lines = h->lines;
	return 0;
}

unsigned long long
mgdk_select_groupsum_last_lines(void)
{
	return gs_last_lines;
}

int
mgdk_avg3_of_sum(const void *sum_hge, int64_t n, int64_t *avg, int64_t *rem)
{
	if (sum_hge == nullptr || avg == nullptr || rem == nullptr || n <= 0)
		return -1;
	hge s;
	memcpy(&s, sum_hge, 16);
	avg3_of_sum(s, n, avg, rem);
	return 0;
}

}  // extern "C"
