// analytic_rank.hip -- the ranking window functions on the MI355X:
// SQLrow_number, SQLrank, SQLdense_rank, SQLpercent_rank and SQLcume_dist
// (sql/backends/monet5/sql_rank.c), the consumers of the partition bits p and
// peer bits o of GDKanalyticaldiff; DESIGN.md 11.7.
//
// The reference walks p and o row by row.  On the device a row needs
//   a  the last partition start at or before it,
//   x  the last peer start at or before it (a partition start is one),
//   d  the peer bits since a (dense_rank),
//   e  the next partition start after it, or the row count,
//   y  the next peer start after it, or the row count,
// which are segmented scans over the two byte columns.  They are computed
// as scans, reduce-then-scan over tiles of 4096 rows in groups of 64 tiles:
//   pass 1   k_rank_tile    one wave per tile: its forward state (RankFwd)
//                           and backward state (RankBwd) from its bytes, 16
//                           bytes per lane, column and load;
//   pass 2a  k_rank_groups  one wave per group: the fold of its tiles;
//   pass 2b  k_rank_tiles   one workgroup: the exclusive prefix (forward) and
//                           suffix (backward) of the group states;
//   pass 3   k_rank_write   one workgroup per tile, 16 rows per lane: folds
//                           the tiles of its group before (after) it onto the
//                           group's prefix (suffix), recomputes its tile from
//                           the bytes, scans the lanes, and writes every
//                           row's result row-wise through LDS (whole 128-byte
//                           lines per store; dbl in two rounds of 2048 rows,
//                           so the LDS is an int tile's).
// No workgroup waits for another.  There is no list of starts and no search:
// the cost per row does not depend on the number of partitions or peer
// groups.  p and o are read twice each, the result is written once, and the
// tile state is 20 bytes per 4096 rows (and 40 per group).
//
// Without o every row of a partition is a peer of every other: rank and
// dense_rank are 1, percent_rank is 0 and cume_dist is 1 whatever p holds, so
// those calls (and row_number without p, an iota) are one fill kernel that
// reads nothing.  Row 0 starts a partition whatever p[0] and o[0] hold; a
// non-zero byte (the nil -128 included) is a set bit.
#include "mgdk_internal.h"
#include "segments.h"

using namespace mgdk;

namespace {

constexpr uint32_t RK_PER = 16, RK_TILE = 256 * RK_PER;
// one pad slot per RK_PER keeps a lane's consecutive writes off a single bank
constexpr uint32_t RK_SLOTS = RK_TILE + RK_TILE / RK_PER;
// tiles per group: one per lane of the wave that folds them
constexpr uint32_t RK_GROUP = 64;

enum { RK_ROWNUM = 0, RK_RANK = 1, RK_DENSE = 2, RK_PERCENT = 3, RK_CUME = 4 };

// ---- the combines -----------------------------------------------------------
// Forward state of a run of consecutive rows.  Positions are stored as row +
// 1, 0: the run holds none.  ls counts partition starts as peer starts; dn
// counts the rows with o set and p clear after the run's last partition start
// (all of them when it holds none).  Associative, not commutative: the right
// operand is the later run.
struct RankFwd {
	uint32_t lp;    // last partition start
	uint32_t ls;    // last peer start
	uint32_t dn;    // peer bits after lp
};

__device__ __forceinline__ RankFwd
rank_fwd_comb(const RankFwd &a, const RankFwd &b)
{
	RankFwd r;
	r.lp = b.lp ? b.lp : a.lp;
	r.ls = b.ls ? b.ls : a.ls;
	r.dn = b.lp ? b.dn : a.dn + b.dn;
	return r;
}

// Backward state of a run: its first partition start and first peer start as
// plain rows, the row count when it holds none, so the combine is a minimum
// and a run after the last start answers "the row count" by itself.
struct RankBwd {
	uint32_t fp;
	uint32_t fs;
};

__device__ __forceinline__ RankBwd
rank_bwd_comb(const RankBwd &a, const RankBwd &b)
{
	return RankBwd{min(a.fp, b.fp), min(a.fs, b.fs)};
}

__device__ __forceinline__ RankFwd
fwd_shfl_up(const RankFwd &s, int d)
{
	return RankFwd{(uint32_t) __shfl_up((int) s.lp, d), (uint32_t) __shfl_up((int) s.ls, d),
		       (uint32_t) __shfl_up((int) s.dn, d)};
}

__device__ __forceinline__ RankBwd
bwd_shfl_down(const RankBwd &s, int d)
{
	return RankBwd{(uint32_t) __shfl_down((int) s.fp, d), (uint32_t) __shfl_down((int) s.fs, d)};
}

// inclusive scan of one forward state per lane of the wave, in lane order
__device__ __forceinline__ RankFwd
fwd_wave_incl(const RankFwd &v)
{
	const unsigned lane = __lane_id();
	RankFwd inc = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const RankFwd y = fwd_shfl_up(inc, d);
		if ((int) lane >= d)
			inc = rank_fwd_comb(y, inc);
	}
	return inc;
}

// the fold of the wave's states in lane order, in every lane
__device__ __forceinline__ RankFwd
fwd_wave_fold(const RankFwd &v)
{
	const RankFwd inc = fwd_wave_incl(v);
	return RankFwd{(uint32_t) __shfl((int) inc.lp, 63), (uint32_t) __shfl((int) inc.ls, 63),
		       (uint32_t) __shfl((int) inc.dn, 63)};
}

// the backward combine is a minimum: any order
__device__ __forceinline__ RankBwd
bwd_wave_fold(const RankBwd &v)
{
	RankBwd r = v;
#pragma unroll
	for (int d = 32; d > 0; d >>= 1)
		r = rank_bwd_comb(r, RankBwd{(uint32_t) __shfl_xor((int) r.fp, d), (uint32_t) __shfl_xor((int) r.fs, d)});
	return r;
}

// exclusive scan of one forward state per thread in thread order (blockDim.x
// a multiple of 64, at most 1024): the wave scans, then the waves' totals
// through LDS
__device__ __forceinline__ RankFwd
fwd_block_excl(const RankFwd &v, RankFwd *wt)
{
	const unsigned lane = __lane_id(), w = threadIdx.x >> 6;
	const RankFwd inc = fwd_wave_incl(v);
	RankFwd ex = fwd_shfl_up(inc, 1);
	if (lane == 0)
		ex = RankFwd{0, 0, 0};
	if (lane == 63)
		wt[w] = inc;
	__syncthreads();
	RankFwd wp{0, 0, 0};
	for (unsigned q = 0; q < w; q++)
		wp = rank_fwd_comb(wp, wt[q]);
	return rank_fwd_comb(wp, ex);
}

// the same from the back: the fold of the threads after this one (none: the
// identity {n, n})
__device__ __forceinline__ RankBwd
bwd_block_excl(const RankBwd &v, uint32_t n, RankBwd *wt)
{
	const unsigned lane = __lane_id(), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
	RankBwd inc = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const RankBwd y = bwd_shfl_down(inc, d);
		if ((int) lane + d < 64)
			inc = rank_bwd_comb(inc, y);
	}
	RankBwd ex = bwd_shfl_down(inc, 1);
	if (lane == 63)
		ex = RankBwd{n, n};
	if (lane == 0)
		wt[w] = inc;
	__syncthreads();
	RankBwd ws{n, n};
	for (unsigned q = w + 1; q < nw; q++)
		ws = rank_bwd_comb(ws, wt[q]);
	return rank_bwd_comb(ex, ws);
}

// ---- a lane's 16 rows -------------------------------------------------------

// bit k = byte k of w is not zero (k = 0..3)
__device__ __forceinline__ uint32_t
nz4(uint32_t w)
{
	const uint32_t t = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
	return (((t >> 7) * 0x00204081u) >> 21) & 0xfu;
}

// bit k = c[r0 + k] is not zero, k = 0..15; rows from n on read as clear.
// wide: c is 16-byte aligned, so the lane's rows are one 16-byte load
__device__ __forceinline__ uint32_t
load_bits(const int8_t *c, uint32_t r0, uint32_t n, bool wide)
{
	if (r0 >= n)
		return 0;
	if (wide && n - r0 >= RK_PER) {
		const uint4 v = *reinterpret_cast<const uint4 *>(c + r0);
		return nz4(v.x) | nz4(v.y) << 4 | nz4(v.z) << 8 | nz4(v.w) << 12;
	}
	uint32_t m = 0;
#pragma unroll
	for (uint32_t k = 0; k < RK_PER; k++)
		if (r0 + k < n && c[r0 + k] != 0)
			m |= 1u << k;
	return m;
}

// the partition bits pm and peer-start bits sm (partition starts included)
// of the lane's rows, and dm: o set and p clear
template <bool HASP, bool HASO>
__device__ __forceinline__ void
lane_bits(const int8_t *p, const int8_t *o, uint32_t r0, uint32_t n, bool wide, uint32_t &pm, uint32_t &sm,
	  uint32_t &dm)
{
	pm = HASP ? load_bits(p, r0, n, wide) : 0;
	const uint32_t om = HASO ? load_bits(o, r0, n, wide) : 0;
	if (r0 == 0)
		pm |= 1;            // row 0 starts a partition
	sm = pm | om;
	dm = om & ~pm;
}

__device__ __forceinline__ uint32_t
top_bit(uint32_t m)
{
	return 31u - (uint32_t) __clz((int) m);
}

__device__ __forceinline__ uint32_t
low_bit(uint32_t m)
{
	return (uint32_t) __ffs((int) m) - 1u;
}

__device__ __forceinline__ RankFwd
lane_fwd(uint32_t r0, uint32_t pm, uint32_t sm, uint32_t dm)
{
	RankFwd f;
	f.lp = pm ? r0 + top_bit(pm) + 1 : 0;
	f.ls = sm ? r0 + top_bit(sm) + 1 : 0;
	f.dn = (uint32_t) __popc(pm ? dm >> (top_bit(pm) + 1) : dm);
	return f;
}

__device__ __forceinline__ RankBwd
lane_bwd(uint32_t r0, uint32_t n, uint32_t pm, uint32_t sm)
{
	return RankBwd{pm ? r0 + low_bit(pm) : n, sm ? r0 + low_bit(sm) : n};
}

// the bits of m (bit k: row r0 + k) at the rows from `from` on
__device__ __forceinline__ uint32_t
bits_from(uint32_t r0, uint32_t m, uint32_t from)
{
	if (from <= r0)
		return (uint32_t) __popc(m);
	const uint32_t s = from - r0;
	return s >= RK_PER ? 0 : (uint32_t) __popc(m >> s);
}

template <typename F>
__device__ __forceinline__ uint32_t
wave_all(uint32_t v, F op)
{
#pragma unroll
	for (int d = 32; d > 0; d >>= 1)
		v = op(v, (uint32_t) __shfl_xor((int) v, d));
	return v;
}

// the states of tile / group i of a table of cnt entries, one array of cnt
// words per field: lp, ls, dn, fp, fs
__device__ __forceinline__ RankFwd
get_fwd(const uint32_t *tab, uint32_t cnt, uint32_t i)
{
	return RankFwd{tab[i], tab[cnt + i], tab[2 * cnt + i]};
}

__device__ __forceinline__ RankBwd
get_bwd(const uint32_t *tab, uint32_t cnt, uint32_t i)
{
	return RankBwd{tab[3 * cnt + i], tab[4 * cnt + i]};
}

__device__ __forceinline__ void
put_fwd(uint32_t *tab, uint32_t cnt, uint32_t i, const RankFwd &f)
{
	tab[i] = f.lp;
	tab[cnt + i] = f.ls;
	tab[2 * cnt + i] = f.dn;
}

__device__ __forceinline__ void
put_bwd(uint32_t *tab, uint32_t cnt, uint32_t i, const RankBwd &b)
{
	tab[3 * cnt + i] = b.fp;
	tab[4 * cnt + i] = b.fs;
}

// ---- pass 1: the tiles' states ------------------------------------------------
// One wave per tile: four rounds of 1024 rows, 16 per lane, loaded before any
// is folded.  A lane's rounds are 1024 rows apart, so the wave does not fold
// in row order: whatever the order, lp and ls are maxima and fp and fs
// minima, and dn -- the peer bits after lp, as rank_fwd_comb leaves it -- is
// counted once the tile's lp is known: three short chains of cross-lane
// moves instead of an ordered wave scan per round
template <bool HASP, bool HASO>
__global__ __launch_bounds__(256) void
k_rank_tile(const int8_t *p, const int8_t *o, uint32_t n, bool wide, uint32_t nt, uint32_t *agg)
{
	constexpr uint32_t ROUNDS = RK_TILE / (64 * RK_PER);
	const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (t >= nt)
		return;             // the whole wave
	const uint32_t r0 = t * RK_TILE + __lane_id() * RK_PER;
	uint32_t pm[ROUNDS], sm[ROUNDS], dm[ROUNDS];
#pragma unroll
	for (uint32_t j = 0; j < ROUNDS; j++)
		lane_bits<HASP, HASO>(p, o, r0 + j * 64 * RK_PER, n, wide, pm[j], sm[j], dm[j]);
	RankFwd tf{0, 0, 0};
	RankBwd tb{n, n};
#pragma unroll
	for (uint32_t j = 0; j < ROUNDS; j++) {
		const uint32_t r = r0 + j * 64 * RK_PER;
		const RankFwd f = lane_fwd(r, pm[j], sm[j], dm[j]);
		tf.lp = max(tf.lp, f.lp);
		tf.ls = max(tf.ls, f.ls);
		tb = rank_bwd_comb(tb, lane_bwd(r, n, pm[j], sm[j]));
	}
	tf.lp = wave_all(tf.lp, [](uint32_t x, uint32_t y) { return max(x, y); });
	tf.ls = wave_all(tf.ls, [](uint32_t x, uint32_t y) { return max(x, y); });
	tb = bwd_wave_fold(tb);
#pragma unroll
	for (uint32_t j = 0; j < ROUNDS; j++)
		tf.dn += bits_from(r0 + j * 64 * RK_PER, dm[j], tf.lp);
	tf.dn = wave_all(tf.dn, [](uint32_t x, uint32_t y) { return x + y; });
	if (__lane_id() == 0) {
		put_fwd(agg, nt, t, tf);
		put_bwd(agg, nt, t, tb);
	}
}

// ---- pass 2a: the groups' states ------------------------------------------------
// One wave per group of RK_GROUP tiles, one tile per lane
__global__ __launch_bounds__(256) void
k_rank_groups(const uint32_t *agg, uint32_t nt, uint32_t n, uint32_t ng, uint32_t *gagg)
{
	const uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (g >= ng)
		return;             // the whole wave
	const uint32_t t = g * RK_GROUP + __lane_id();
	const RankFwd gf = fwd_wave_fold(t < nt ? get_fwd(agg, nt, t) : RankFwd{0, 0, 0});
	const RankBwd gb = bwd_wave_fold(t < nt ? get_bwd(agg, nt, t) : RankBwd{n, n});
	if (__lane_id() == 0) {
		put_fwd(gagg, ng, g, gf);
		put_bwd(gagg, ng, g, gb);
	}
}

// ---- pass 2b: the group of groups -------------------------------------------------
// pre[g] = the fold of the groups before g (forward fields) and of the groups
// after it (backward fields), laid out as gagg is.  One workgroup of 1024
// threads: thread t folds RK_TPT consecutive groups, one block scan of
// those, then it writes its groups' prefixes.  2^31 rows are 8192 groups:
// one round; the loops carry a round into the next all the same
constexpr uint32_t RK_TPT = 8;

__global__ __launch_bounds__(1024) void
k_rank_tiles(const uint32_t *gagg, uint32_t ng, uint32_t n, uint32_t *pre)
{
	__shared__ RankFwd wf[16], cfwd;
	__shared__ RankBwd wb[16], cbwd;
	const uint32_t round = 1024 * RK_TPT;
	RankFwd carry{0, 0, 0};
	for (uint32_t g0 = 0; g0 < ng; g0 += round) {
		const uint32_t b0 = g0 + threadIdx.x * RK_TPT;
		RankFwd v[RK_TPT], acc{0, 0, 0};
#pragma unroll
		for (uint32_t k = 0; k < RK_TPT; k++) {
			v[k] = b0 + k < ng ? get_fwd(gagg, ng, b0 + k) : RankFwd{0, 0, 0};
			acc = rank_fwd_comb(acc, v[k]);
		}
		RankFwd run = rank_fwd_comb(carry, fwd_block_excl(acc, wf));
#pragma unroll
		for (uint32_t k = 0; k < RK_TPT; k++) {
			if (b0 + k < ng)
				put_fwd(pre, ng, b0 + k, run);
			run = rank_fwd_comb(run, v[k]);
		}
		// the last thread's run is now the fold of the whole round
		if (threadIdx.x == 1023)
			cfwd = run;
		__syncthreads();
		carry = cfwd;
		__syncthreads();
	}
	RankBwd back{n, n};
	const uint32_t nr = (ng + round - 1) / round;
	for (uint32_t rr = nr; rr-- > 0;) {
		const uint32_t b0 = rr * round + threadIdx.x * RK_TPT;
		RankBwd v[RK_TPT], acc{n, n};
#pragma unroll
		for (uint32_t k = 0; k < RK_TPT; k++) {
			v[k] = b0 + k < ng ? get_bwd(gagg, ng, b0 + k) : RankBwd{n, n};
			acc = rank_bwd_comb(acc, v[k]);
		}
		RankBwd run = rank_bwd_comb(bwd_block_excl(acc, n, wb), back);
#pragma unroll
		for (int k = (int) RK_TPT - 1; k >= 0; k--) {
			if (b0 + k < ng)
				put_bwd(pre, ng, b0 + k, run);
			run = rank_bwd_comb(v[k], run);
		}
		// and the first thread's the fold of this round and the later ones
		if (threadIdx.x == 0)
			cbwd = run;
		__syncthreads();
		back = cbwd;
		__syncthreads();
	}
}

// ---- pass 3: the results ------------------------------------------------------

template <int FN> struct RankOut { typedef int32_t T; };
template <> struct RankOut<RK_PERCENT> { typedef double T; };
template <> struct RankOut<RK_CUME> { typedef double T; };

template <int FN, bool HASP, bool HASO>
__global__ __launch_bounds__(256) void
k_rank_write(const int8_t *p, const int8_t *o, uint32_t n, bool wide, uint32_t nt, const uint32_t *agg, uint32_t ng,
	     const uint32_t *gpre, typename RankOut<FN>::T *out)
{
	typedef typename RankOut<FN>::T T;
	constexpr bool BACK = FN == RK_PERCENT || FN == RK_CUME;
	// the results go out in rounds of as many rows as fill the LDS of an int
	// tile: one round for int, two for dbl (the first two waves' rows, then
	// the others')
	constexpr uint32_t OUT_ROUNDS = sizeof(T) / sizeof(int32_t), OUT_THREADS = 256 / OUT_ROUNDS,
			   OUT_ROWS = RK_TILE / OUT_ROUNDS;
	__shared__ RankFwd wf[4];
	__shared__ RankBwd wb[4];
	__shared__ T wo[RK_SLOTS / OUT_ROUNDS];
	const uint32_t t0 = blockIdx.x * RK_TILE, l0 = threadIdx.x * RK_PER, r0 = t0 + l0;
	// the states of the group's tiles before / after this one, one per lane
	// (every wave folds them itself), and of the groups before / after it:
	// loaded ahead of the tile's bytes
	const uint32_t g = blockIdx.x / RK_GROUP, tl = blockIdx.x % RK_GROUP, tw = g * RK_GROUP + __lane_id();
	const RankFwd gf = get_fwd(gpre, ng, g);
	const RankFwd af = __lane_id() < tl ? get_fwd(agg, nt, tw) : RankFwd{0, 0, 0};
	RankBwd gb{n, n}, ab{n, n};
	if (BACK) {
		gb = get_bwd(gpre, ng, g);
		if (__lane_id() > tl && tw < nt)
			ab = get_bwd(agg, nt, tw);
	}
	uint32_t pm, sm, dm;
	lane_bits<HASP, HASO>(p, o, r0, n, wide, pm, sm, dm);
	// the state before the lane's first row: the tiles before, the lanes before
	const RankFwd tpre = rank_fwd_comb(gf, fwd_wave_fold(af));
	const RankFwd cf = rank_fwd_comb(tpre, fwd_block_excl(lane_fwd(r0, pm, sm, dm), wf));
	RankBwd cb{n, n};
	if (BACK) {
		const RankBwd tnxt = rank_bwd_comb(bwd_wave_fold(ab), gb);
		cb = rank_bwd_comb(bwd_block_excl(lane_bwd(r0, n, pm, sm), n, wb), tnxt);
	}
	T res[RK_PER];
#pragma unroll
	for (uint32_t k = 0; k < RK_PER; k++) {
		const uint32_t row = r0 + k, upto = (2u << k) - 1;
		const uint32_t pl = pm & upto, sl = sm & upto, dl = dm & upto;
		const uint32_t a = pl ? r0 + top_bit(pl) : cf.lp - 1;
		const uint32_t x = sl ? r0 + top_bit(sl) : cf.ls - 1;
		T v;
		if (FN == RK_ROWNUM) {
			v = (T) (row - a + 1);
		} else if (FN == RK_RANK) {
			v = (T) (x - a + 1);
		} else if (FN == RK_DENSE) {
			v = (T) ((pl ? (uint32_t) __popc(dl >> (top_bit(pl) + 1)) : cf.dn + (uint32_t) __popc(dl)) + 1);
		} else {
			const uint32_t ph = pm >> (k + 1), sh = sm >> (k + 1);
			const uint32_t e = ph ? row + 1 + low_bit(ph) : cb.fp;
			const uint32_t cnt = e - a;
			if (FN == RK_PERCENT) {
				v = cnt == 1 ? (T) 0 : (T) ((double) (x - a) / (double) (cnt - 1));
			} else {
				const uint32_t y = sh ? row + 1 + low_bit(sh) : cb.fs;
				v = (T) ((double) (y - a) / (double) cnt);
			}
		}
		res[k] = v;
	}
	const uint32_t tend = n - t0 < RK_TILE ? n - t0 : RK_TILE;
#pragma unroll
	for (uint32_t h = 0; h < OUT_ROUNDS; h++) {
		if (h)
			__syncthreads();      // the round before has been read
		if (threadIdx.x / OUT_THREADS == h) {
			// slot i + i / RK_PER of the round's row i
			const uint32_t lt = threadIdx.x - h * OUT_THREADS;
#pragma unroll
			for (uint32_t k = 0; k < RK_PER; k++)
				wo[lt * RK_PER + k + lt] = res[k];
		}
		__syncthreads();
#pragma unroll
		for (uint32_t k = 0; k < RK_PER / OUT_ROUNDS; k++) {
			const uint32_t i = k * 256 + threadIdx.x, row = h * OUT_ROWS + i;
			if (row < tend)
				out[t0 + row] = wo[i + i / RK_PER];
		}
	}
}

// the calls that read no column: one value for every row, or 1, 2, 3, ...
template <typename T, bool IOTA>
__global__ __launch_bounds__(256) void
k_rank_fill(T *out, uint32_t n, T v)
{
	for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
		out[i] = IOTA ? (T) (i + 1) : v;
}

// ---- host side ------------------------------------------------------------------

template <int FN, bool HASP, bool HASO>
void
launch_write(const int8_t *p, const int8_t *o, uint32_t n, bool wide, uint32_t nt, const uint32_t *agg, uint32_t ng,
	     const uint32_t *gpre, void *out)
{
	hipLaunchKernelGGL((k_rank_write<FN, HASP, HASO>), dim3(nt), dim3(256), 0, stream(), p, o, n, wide, nt, agg, ng,
			   gpre, (typename RankOut<FN>::T *) out);
}

template <bool HASP, bool HASO>
void
launch_scan(int fn, const int8_t *p, const int8_t *o, uint32_t n, bool wide, uint32_t nt, uint32_t *agg,
	    void *out)
{
	// the table of tile states, then the groups' states and their prefixes
	const uint32_t ng = (nt + RK_GROUP - 1) / RK_GROUP;
	uint32_t *gagg = agg + (size_t) 5 * nt, *gpre = gagg + (size_t) 5 * ng;
	hipStream_t st = stream();
	hipLaunchKernelGGL((k_rank_tile<HASP, HASO>), dim3((nt + 3) / 4), dim3(256), 0, st, p, o, n, wide, nt, agg);
	hipLaunchKernelGGL(k_rank_groups, dim3((ng + 3) / 4), dim3(256), 0, st, agg, nt, n, ng, gagg);
	hipLaunchKernelGGL(k_rank_tiles, dim3(1), dim3(1024), 0, st, gagg, ng, n, gpre);
	// row_number comes here with p alone, the other four only with o
	if constexpr (!HASO) {
		launch_write<RK_ROWNUM, HASP, HASO>(p, o, n, wide, nt, agg, ng, gpre, out);
	} else {
		switch (fn) {
		case RK_RANK: launch_write<RK_RANK, HASP, HASO>(p, o, n, wide, nt, agg, ng, gpre, out); break;
		case RK_DENSE: launch_write<RK_DENSE, HASP, HASO>(p, o, n, wide, nt, agg, ng, gpre, out); break;
		case RK_PERCENT: launch_write<RK_PERCENT, HASP, HASO>(p, o, n, wide, nt, agg, ng, gpre, out); break;
		default: launch_write<RK_CUME, HASP, HASO>(p, o, n, wide, nt, agg, ng, gpre, out); break;
		}
	}
}

mgdk_bat *
rank_run(int fn, mgdk_bat *b, mgdk_bat *p, mgdk_bat *o, const char *name)
{
	if (b == nullptr) {
		seterr("%s: NULL argument", name);
		return nullptr;
	}
	const BUN cnt = b->count;
	if (cnt > (BUN) INT32_MAX) {
		// the reference counts rows in an int, which wraps here
		seterr("42000!%s: more than 2^31 - 1 rows not supported on the device path", name);
		return nullptr;
	}
	if (!bits_ok(p, cnt, true) || !bits_ok(o, cnt, true))
		return nullptr;
	const bool dbl = fn == RK_PERCENT || fn == RK_CUME;
	mgdk_bat *r = newbat(b->hseqbase, dbl ? MGDK_dbl : MGDK_int, cnt);
	if (r == nullptr)
		return nullptr;
	const uint32_t n = (uint32_t) cnt;
	if (n > 0) {
		// row_number has no peers; without o every row of a partition is a
		// peer of the others and the other four do not depend on p
		const int8_t *pp = p && (fn == RK_ROWNUM || o) ? (const int8_t *) p->theap : nullptr;
		const int8_t *oo = o && fn != RK_ROWNUM ? (const int8_t *) o->theap : nullptr;
		hipStream_t st = stream();
		if (pp == nullptr && oo == nullptr) {
			const dim3 g(grid_for(n, 1024, 8192)), blk(256);
			if (fn == RK_ROWNUM)
				hipLaunchKernelGGL((k_rank_fill<int32_t, true>), g, blk, 0, st, (int32_t *) r->theap, n, 0);
			else if (!dbl)
				hipLaunchKernelGGL((k_rank_fill<int32_t, false>), g, blk, 0, st, (int32_t *) r->theap, n, 1);
			else
				hipLaunchKernelGGL((k_rank_fill<double, false>), g, blk, 0, st, (double *) r->theap, n,
						   fn == RK_CUME ? 1.0 : 0.0);
			if (!sync()) {
				mgdk_BBPunfix(r);
				return nullptr;
			}
		} else {
			const uint32_t nt = (n + RK_TILE - 1) / RK_TILE;
			const uint32_t ng = (nt + RK_GROUP - 1) / RK_GROUP;
			DevBuf tiles(((size_t) nt + 2 * (size_t) ng) * 5 * sizeof(uint32_t));
			if (tiles.p == nullptr) {
				mgdk_BBPunfix(r);
				return nullptr;
			}
			uint32_t *agg = tiles.as<uint32_t>();
			// a view (BATslice) may start anywhere: its rows then load bytewise
			const bool wide = (((uintptr_t) pp | (uintptr_t) oo) & 15) == 0;
			if (pp && oo)
				launch_scan<true, true>(fn, pp, oo, n, wide, nt, agg, r->theap);
			else if (pp)
				launch_scan<true, false>(fn, pp, oo, n, wide, nt, agg, r->theap);
			else
				launch_scan<false, true>(fn, pp, oo, n, wide, nt, agg, r->theap);
			if (!sync()) {
				mgdk_BBPunfix(r);
				return nullptr;
			}
		}
	}
	r->count = cnt;
	r->tnonil = 1;
	r->tnil = 0;
	r->tsorted = r->trevsorted = r->tkey = cnt <= 1;
	return r;
}

}  // namespace

extern "C" mgdk_bat *
mgdk_SQLrow_number(mgdk_bat *b, mgdk_bat *p)
{
	ProfScope prof("sqlrow_number");
	return rank_run(RK_ROWNUM, b, p, nullptr, "SQLrow_number");
}

extern "C" mgdk_bat *
mgdk_SQLrank(mgdk_bat *b, mgdk_bat *p, mgdk_bat *o)
{
	ProfScope prof("sqlrank");
	return rank_run(RK_RANK, b, p, o, "SQLrank");
}

extern "C" mgdk_bat *
mgdk_SQLdense_rank(mgdk_bat *b, mgdk_bat *p, mgdk_bat *o)
{
	ProfScope prof("sqldense_rank");
	return rank_run(RK_DENSE, b, p, o, "SQLdense_rank");
}

extern "C" mgdk_bat *
mgdk_SQLpercent_rank(mgdk_bat *b, mgdk_bat *p, mgdk_bat *o)
{
	ProfScope prof("sqlpercent_rank");
	return rank_run(RK_PERCENT, b, p, o, "SQLpercent_rank");
}

extern "C" mgdk_bat *
mgdk_SQLcume_dist(mgdk_bat *b, mgdk_bat *p, mgdk_bat *o)
{
	ProfScope prof("sqlcume_dist");
	return rank_run(RK_CUME, b, p, o, "SQLcume_dist");
}
