// runscan.h -- the parallel form of a running fold over the peer runs of a
// partition (frames 3 / 4, and frame 5 through its first two passes), shared
// by GDKanalyticalsum, GDKanalyticalavg (analytic_func.hip) and the window
// statistics (analytic_stats.hip); DESIGN.md 11.5.
//
// Positions q are rows in fold order (frame 3: q = row; frame 4: q = n - 1 -
// row); a position ends its peer run where the replay writes (frame 3:
// o[row + 1] or the last row; frame 4: o[row] or row 0; without o only the
// last position).  Pass 1 folds each 4096-position tile (16 per lane, the
// lanes combined in order); pass 2 scans the tile totals; pass 3 writes every
// position's result; pass 4 gives every position the result at the end of its
// run (end positions are never rewritten, so it reads them in place).  Frame
// 5 takes the partition's total from passes 1 and 2 and broadcasts its result.
//
// The fold is a policy P, passed to the kernels by value:
//   State, Out, Raw      the scanned state, the output element, a row's value(s)
//   Stage                a tile's raw values in LDS, RS_SLOTS slots
//   TPT                  tile totals per thread and round of pass 2 (registers)
//   stage(sg, slot, row) / stage_none(sg, slot)   global -> LDS
//   raw(sg, slot)        LDS -> registers
//   leaf(raw, valid)     the state of one position (valid: inside the partition)
//   zero(), comb(a, b, fl), shfl_up(s, d)         the ordered combine
//   result(s, end, fl)   the value written for a position (end: it ends a run;
//                        only those values survive pass 4)
// Only the rounding differs from the sequential fold.
#pragma once

#include "mgdk_internal.h"
#include "segments.h"

namespace mgdk {

constexpr unsigned RS_PER = 16, RS_TILE = 256 * RS_PER;
// one pad slot per RS_PER keeps a lane's consecutive reads off a single bank
constexpr unsigned RS_SLOTS = RS_TILE + RS_TILE / RS_PER;

__device__ __forceinline__ unsigned
rs_slot(unsigned i)
{
	return i + i / RS_PER;
}

__device__ __forceinline__ BUN
rs_row(BUN q, BUN n, bool fwd)
{
	return fwd ? q : n - 1 - q;
}

// a tile's values and end bytes, loaded row-wise (consecutive lanes,
// consecutive addresses); each lane then reads its RS_PER consecutive
// positions
template <typename P>
struct RsStage {
	typename P::Stage v;
	int8_t f[RS_TILE];
};

// a lane's RS_PER positions q0 .. q0 + RS_PER - 1 of its tile: raw values and
// run-end flags.  base: the partition's first row, o: its peer bytes (or NULL)
template <typename P>
__device__ __forceinline__ void
rs_load(const P &p, BUN base, const int8_t *o, BUN n, bool fwd, BUN tb, RsStage<P> &sg,
	typename P::Raw (&x)[RS_PER], bool (&e)[RS_PER])
{
	const BUN t0 = tb * RS_TILE;
#pragma unroll
	for (unsigned k = 0; k < RS_PER; k++) {
		const unsigned i = k * 256 + threadIdx.x;
		const BUN q = t0 + i;
		int8_t f = 1;
		if (q < n) {
			p.stage(sg.v, rs_slot(i), base + rs_row(q, n, fwd));
			// the end flag's byte: o[q + 1] (frame 3) or o[n - 1 - q] (frame
			// 4); the last position always ends its run
			if (q + 1 < n)
				f = o ? o[fwd ? q + 1 : n - 1 - q] : 0;
		} else {
			p.stage_none(sg.v, rs_slot(i));
		}
		sg.f[i] = f;
	}
	__syncthreads();
	const unsigned l0 = threadIdx.x * RS_PER;
#pragma unroll
	for (unsigned k = 0; k < RS_PER; k++) {
		const unsigned i = l0 + k;
		x[k] = p.raw(sg.v, rs_slot(i));
		e[k] = t0 + i < n && sg.f[i] != 0;
	}
}

// ordered exclusive scan over the block's values (blockDim.x a multiple of
// 64, at most 1024): a wave scan by shuffles, then the waves' totals through
// LDS (one barrier); the same association every launch.  *total = the fold
// of all of them
template <typename P>
__device__ __forceinline__ typename P::State
rs_block_excl(typename P::State v, typename P::State *wt, uint32_t &fl, typename P::State *total)
{
	using S = typename P::State;
	const unsigned lane = __lane_id(), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
	S inc = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const S y = P::shfl_up(inc, d);
		if ((int) lane >= d)
			inc = P::comb(y, inc, fl);
	}
	S ex = P::shfl_up(inc, 1);
	if (lane == 0)
		ex = P::zero();
	if (lane == 63)
		wt[w] = inc;
	__syncthreads();
	S wp = P::zero(), all = P::zero();
	for (unsigned q = 0; q < nw; q++) {
		if (q < w)
			wp = P::comb(wp, wt[q], fl);
		all = P::comb(all, wt[q], fl);
	}
	*total = all;
	__syncthreads();            // wt may be reused by the caller
	return P::comb(wp, ex, fl);
}

// pass 1 (tb: the tile's index within its partition, slot: its place in tot /
// fend; the same number with one partition)
template <typename P>
__device__ __forceinline__ void
rs_tile_body(const P &p, BUN base, const int8_t *o, BUN n, bool fwd, BUN tb, BUN slot, typename P::State *tot,
	     BUN *fend, uint32_t *flags)
{
	using S = typename P::State;
	__shared__ S wt[16];
	__shared__ BUN sm[4];
	__shared__ RsStage<P> sg;
	const BUN q0 = tb * RS_TILE + threadIdx.x * RS_PER;
	typename P::Raw x[RS_PER];
	bool e[RS_PER];
	rs_load<P>(p, base, o, n, fwd, tb, sg, x, e);
	S acc = P::zero();
	BUN fe = ~(BUN) 0;
	uint32_t fl = 0;
#pragma unroll
	for (int k = (int) RS_PER - 1; k >= 0; k--)
		if (e[k])
			fe = q0 + k;
#pragma unroll
	for (unsigned k = 0; k < RS_PER; k++)
		acc = P::comb(acc, p.leaf(x[k], q0 + k < n), fl);
	S total;
	(void) rs_block_excl<P>(acc, wt, fl, &total);
#pragma unroll
	for (int d = 32; d > 0; d >>= 1)
		fe = min(fe, (BUN) __shfl_xor(fe, d));
	if (__lane_id() == 0)
		sm[threadIdx.x >> 6] = fe;
	__syncthreads();
	fe = min(min(sm[0], sm[1]), min(sm[2], sm[3]));
	if (threadIdx.x == 0) {
		tot[slot] = total;
		fend[slot] = fe;
	}
	if (fl)
		atomicOr(flags, fl);
}

template <typename P>
__global__ __launch_bounds__(256) void
k_rs_tile(P p, const int8_t *o, BUN n, bool fwd, typename P::State *tot, BUN *fend, uint32_t *flags)
{
	rs_tile_body<P>(p, 0, o, n, fwd, blockIdx.x, blockIdx.x, tot, fend, flags);
}

// the same over the flat tile table of the large partitions: a tile's
// positions are counted within its partition (frame 4 backwards within it),
// whose first row (frame 4) or last row (frame 3) ends a run
template <typename P>
__global__ __launch_bounds__(256) void
k_rs_tile_seg(P p, const int8_t *o, bool fwd, const FpSeg *segs, const FpTile *tiles, typename P::State *tot,
	      BUN *fend, uint32_t *flags)
{
	const FpTile t = tiles[blockIdx.x];
	const FpSeg sg = segs[t.seg];
	rs_tile_body<P>(p, sg.first, o ? o + sg.first : nullptr, sg.len, fwd, t.tix, blockIdx.x, tot, fend, flags);
}

// pass 2: pre[t] = the fold of the tiles before t (in order); nxt[t] = the
// first run end at or after tile t + 1's first position.  One workgroup of
// 1024 threads: thread t folds a contiguous run of P::TPT tiles (its loads
// issued together), one block scan of the runs, then each thread writes its
// run's prefixes; the suffix minima alike
template <typename P>
__device__ __forceinline__ void
rs_tiles_body(const typename P::State *tot, const BUN *fend, BUN nt, typename P::State *pre, BUN *nxt,
	      uint32_t *flags)
{
	using S = typename P::State;
	constexpr unsigned TPT = P::TPT;
	__shared__ S wt[16];
	__shared__ BUN wm[16];
	uint32_t fl = 0;
	S carry = P::zero();
	const BUN round = (BUN) 1024 * TPT;
	for (BUN r0 = 0; r0 < nt; r0 += round) {
		const BUN b0 = r0 + (BUN) threadIdx.x * TPT;
		S v[TPT];
#pragma unroll
		for (unsigned k = 0; k < TPT; k++) {
			if (b0 + k < nt)
				v[k] = tot[b0 + k];
			else
				v[k] = P::zero();
		}
		S acc = P::zero();
#pragma unroll
		for (unsigned k = 0; k < TPT; k++)
			acc = P::comb(acc, v[k], fl);
		S total;
		S run = P::comb(carry, rs_block_excl<P>(acc, wt, fl, &total), fl);
#pragma unroll
		for (unsigned k = 0; k < TPT; k++) {
			if (b0 + k < nt)
				pre[b0 + k] = run;
			run = P::comb(run, v[k], fl);
		}
		carry = P::comb(carry, total, fl);
	}
	// suffix minima of the first ends, rounds from the back
	BUN m = ~(BUN) 0;
	const BUN nr = (nt + round - 1) / round;
	const unsigned lane = __lane_id(), w = threadIdx.x >> 6;
	for (BUN rr = nr; rr-- > 0;) {
		const BUN b0 = rr * round + (BUN) threadIdx.x * TPT;
		BUN f[TPT];
		BUN own = ~(BUN) 0;
#pragma unroll
		for (unsigned k = 0; k < TPT; k++) {
			f[k] = b0 + k < nt ? fend[b0 + k] : ~(BUN) 0;
			own = min(own, f[k]);
		}
		// minimum over the threads after this one: wave suffix minimum,
		// then the later waves
		BUN suf = own;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const BUN y = (BUN) __shfl_down(suf, d);
			if ((int) lane + d < 64)
				suf = min(suf, y);
		}
		if (lane == 0)
			wm[w] = suf;
		__syncthreads();
		BUN later = m;
		for (unsigned q = w + 1; q < 16; q++)
			later = min(later, wm[q]);
		const BUN nextin = (BUN) __shfl_down(suf, 1);
		BUN after = lane + 1 < 64 ? min(nextin, later) : later;
		const BUN rmin = min(min(min(wm[0], wm[1]), min(wm[2], wm[3])),
				     min(min(min(wm[4], wm[5]), min(wm[6], wm[7])),
					 min(min(min(wm[8], wm[9]), min(wm[10], wm[11])),
					     min(min(wm[12], wm[13]), min(wm[14], wm[15])))));
		__syncthreads();
#pragma unroll
		for (int k = (int) TPT - 1; k >= 0; k--) {
			if (b0 + k < nt)
				nxt[b0 + k] = after;
			after = min(after, f[k]);
		}
		m = min(m, rmin);
	}
	if (fl)
		atomicOr(flags, fl);
}

template <typename P>
__global__ __launch_bounds__(1024) void
k_rs_tiles(const typename P::State *tot, const BUN *fend, BUN nt, typename P::State *pre, BUN *nxt,
	   uint32_t *flags)
{
	rs_tiles_body<P>(tot, fend, nt, pre, nxt, flags);
}

// one workgroup per large partition: the scan restarts at its first tile
template <typename P>
__global__ __launch_bounds__(1024) void
k_rs_tiles_seg(const FpSeg *segs, const typename P::State *tot, const BUN *fend, typename P::State *pre, BUN *nxt,
	       uint32_t *flags)
{
	const FpSeg sg = segs[blockIdx.x];
	rs_tiles_body<P>(tot + sg.tile0, fend + sg.tile0, sg.nb, pre + sg.tile0, nxt + sg.tile0, flags);
}

// pass 3: every position's value -- the result at the end of its peer run
// when that end lies inside the tile (read back from LDS), else its own for
// now -- stored row-wise; pass 4 gives the positions of the tile's open last
// run (its end in a later tile) that end's value, read from the output in
// place (end positions are never rewritten).  out: the partition's first slot
template <typename P>
__device__ __forceinline__ void
rs_write_body(const P &p, BUN base, const int8_t *o, BUN n, bool fwd, BUN tb, BUN slot,
	      const typename P::State *pre, const BUN *nxt, int pass, typename P::Out *out, uint32_t *flags)
{
	using S = typename P::State;
	using Out = typename P::Out;
	__shared__ S ls[16];
	__shared__ BUN lm[256];
	// the staged inputs are in registers before the results are laid out,
	// so both use the same LDS
	constexpr size_t SB = sizeof(RsStage<P>) > sizeof(Out) * RS_SLOTS ? sizeof(RsStage<P>) : sizeof(Out) * RS_SLOTS;
	__shared__ __attribute__((aligned(16))) char buf[SB];
	RsStage<P> &sg = *reinterpret_cast<RsStage<P> *>(buf);
	Out *wo = reinterpret_cast<Out *>(buf);
	const BUN t0 = tb * RS_TILE;
	const BUN q0 = t0 + threadIdx.x * RS_PER;
	const BUN tend = t0 + RS_TILE < n ? t0 + RS_TILE : n;
	uint32_t fl = 0;
	typename P::Raw x[RS_PER];
	bool e[RS_PER];
	rs_load<P>(p, base, o, n, fwd, tb, sg, x, e);
	// the first run end at or after each lane's chunk, inside the tile
	BUN fe = ~(BUN) 0;
#pragma unroll
	for (int k = (int) RS_PER - 1; k >= 0; k--)
		if (e[k])
			fe = q0 + k;
	lm[threadIdx.x] = fe;
	__syncthreads();
	for (unsigned d = 1; d < 256; d <<= 1) {
		BUN y = lm[threadIdx.x];
		if (threadIdx.x + d < 256)
			y = min(y, lm[threadIdx.x + d]);
		__syncthreads();
		lm[threadIdx.x] = y;
		__syncthreads();
	}
	const BUN after = threadIdx.x + 1 < 256 ? lm[threadIdx.x + 1] : ~(BUN) 0;
	if (pass == 1) {
		// the open last run: positions whose end is in a later tile
		BUN endq = after != ~(BUN) 0 ? after : nxt[slot];
		if (after != ~(BUN) 0)
			return;      // this lane's positions all end inside the tile
#pragma unroll
		for (int k = (int) RS_PER - 1; k >= 0; k--) {
			const BUN q = q0 + k;
			if (q >= n)
				continue;
			if (e[k])
				return;      // this position and the ones before it end inside the tile
			out[rs_row(q, n, fwd)] = out[rs_row(endq, n, fwd)];
		}
		return;
	}
	S acc = P::zero();
#pragma unroll
	for (unsigned k = 0; k < RS_PER; k++)
		acc = P::comb(acc, p.leaf(x[k], q0 + k < n), fl);
	S total;
	const S ex = rs_block_excl<P>(acc, ls, fl, &total);
	S run = P::comb(pre[slot], ex, fl);
	const unsigned l0 = threadIdx.x * RS_PER;
#pragma unroll
	for (unsigned k = 0; k < RS_PER; k++) {
		run = P::comb(run, p.leaf(x[k], q0 + k < n), fl);
		wo[rs_slot(l0 + k)] = p.result(run, e[k], fl);
	}
	__syncthreads();
	// positions take their run end's value when it is in the tile (end
	// positions keep their own: nothing they read is rewritten)
	BUN endq = after;
#pragma unroll
	for (int k = (int) RS_PER - 1; k >= 0; k--) {
		const BUN q = q0 + k;
		if (e[k]) {
			endq = q;
			continue;
		}
		if (endq != ~(BUN) 0 && q < n)
			wo[rs_slot(l0 + k)] = wo[rs_slot((unsigned) (endq - t0))];
	}
	__syncthreads();
#pragma unroll
	for (unsigned k = 0; k < RS_PER; k++) {
		const unsigned i = k * 256 + threadIdx.x;
		if (t0 + i < tend)
			out[rs_row(t0 + i, n, fwd)] = wo[rs_slot(i)];
	}
	if (fl)
		atomicOr(flags, fl);
}

template <typename P>
__global__ __launch_bounds__(256) void
k_rs_write(P p, const int8_t *o, BUN n, bool fwd, const typename P::State *pre, const BUN *nxt, int pass,
	   typename P::Out *out, uint32_t *flags)
{
	rs_write_body<P>(p, 0, o, n, fwd, blockIdx.x, blockIdx.x, pre, nxt, pass, out, flags);
}

template <typename P>
__global__ __launch_bounds__(256) void
k_rs_write_seg(P p, const int8_t *o, bool fwd, const FpSeg *segs, const FpTile *tiles, const typename P::State *pre,
	       const BUN *nxt, int pass, typename P::Out *out, uint32_t *flags)
{
	const FpTile t = tiles[blockIdx.x];
	const FpSeg sg = segs[t.seg];
	rs_write_body<P>(p, sg.first, o ? o + sg.first : nullptr, sg.len, fwd, t.tix, blockIdx.x, pre, nxt, pass,
			 out + sg.first, flags);
}

// frame 5: the partition's total (the tiles before its last one, then that
// one), its result taken once per tile and written to the tile's rows
template <typename P>
__global__ __launch_bounds__(256) void
k_rs_bcast_seg(P p, const FpSeg *segs, const FpTile *tiles, const typename P::State *tot,
	       const typename P::State *pre, typename P::Out *out, uint32_t *flags)
{
	const FpTile t = tiles[blockIdx.x];
	const FpSeg sg = segs[t.seg];
	const BUN last = sg.tile0 + sg.nb - 1;
	uint32_t fl = 0;
	const typename P::State all = P::comb(pre[last], tot[last], fl);
	const typename P::Out w = p.result(all, true, fl);
	const BUN t0 = (BUN) t.tix * RS_TILE, tend = t0 + RS_TILE < sg.len ? t0 + RS_TILE : sg.len;
	for (BUN q = t0 + threadIdx.x; q < tend; q += 256)
		out[sg.first + q] = w;
	if (fl && t.tix == 0 && threadIdx.x == 0)
		atomicOr(flags, fl);
}

// the partitions' offsets (m + 1 of them) for fp_large_segments
static __global__ __launch_bounds__(256) void
k_part_offsets(Starts part, uint64_t *off)
{
	for (BUN k = (BUN) blockIdx.x * blockDim.x + threadIdx.x; k <= part.m; k += (BUN) gridDim.x * blockDim.x)
		off[k] = k < part.m ? part.at(k) : part.n;
}

// one partition of n rows in the parallel form (frames 3 / 4)
template <typename P>
int
rs_run_par(const P &p, const int8_t *o, BUN n, bool fwd, typename P::Out *out, uint32_t *flags)
{
	using S = typename P::State;
	hipStream_t st = stream();
	const BUN nt = (n + RS_TILE - 1) / RS_TILE;
	if (nt > 0xffffffffull) {
		seterr("42000!analytic: too many rows on the device path\n");
		return -1;
	}
	DevBuf tot(nt * sizeof(S)), pre(nt * sizeof(S)), fend(nt * sizeof(BUN)), nxt(nt * sizeof(BUN));
	if (!tot.p || !pre.p || !fend.p || !nxt.p)
		return -1;
	hipLaunchKernelGGL((k_rs_tile<P>), dim3((unsigned) nt), dim3(256), 0, st, p, o, n, fwd, tot.as<S>(),
			   fend.as<BUN>(), flags);
	hipLaunchKernelGGL((k_rs_tiles<P>), dim3(1), dim3(1024), 0, st, tot.as<S>(), fend.as<BUN>(), nt, pre.as<S>(),
			   nxt.as<BUN>(), flags);
	hipLaunchKernelGGL((k_rs_write<P>), dim3((unsigned) nt), dim3(256), 0, st, p, o, n, fwd, pre.as<S>(),
			   nxt.as<BUN>(), 0, out, flags);
	hipLaunchKernelGGL((k_rs_write<P>), dim3((unsigned) nt), dim3(256), 0, st, p, o, n, fwd, pre.as<S>(),
			   nxt.as<BUN>(), 1, out, flags);
	return sync() ? 0 : -1;
}

// the partitions of at least par_min rows, which the replay left out, in the
// parallel form: frames 3 / 4 (whole = false) the four passes over the flat
// tile table of RS_TILE-position tiles that never straddle a partition
// start; frame 5 (whole = true, o NULL) passes 1 and 2 and the broadcast
template <typename P>
int
rs_run_large(const P &p, const Starts &part, const int8_t *o, BUN n, BUN par_min, bool fwd, bool whole,
	     typename P::Out *out, uint32_t *flags)
{
	using S = typename P::State;
	hipStream_t st = stream();
	FpSegs ls;
	DevBuf off((part.m + 1) * 8);
	if (!off.p)
		return -1;
	hipLaunchKernelGGL(k_part_offsets, dim3(grid_for(part.m + 1, 1024, 1024)), dim3(256), 0, st, part,
			   off.as<uint64_t>());
	if (fp_large_segments(off.as<uint64_t>(), part.m, n, par_min, ls, RS_TILE) != 0 || ls.nseg == 0)
		return -1;
	const BUN nt = ls.ntile;
	DevBuf tot(nt * sizeof(S)), pre(nt * sizeof(S)), fend(nt * sizeof(BUN)), nxt(nt * sizeof(BUN));
	if (!tot.p || !pre.p || !fend.p || !nxt.p)
		return -1;
	const dim3 tg((unsigned) nt), tb(256);
	hipLaunchKernelGGL((k_rs_tile_seg<P>), tg, tb, 0, st, p, o, fwd, ls.segs, ls.tiles, tot.as<S>(), fend.as<BUN>(),
			   flags);
	hipLaunchKernelGGL((k_rs_tiles_seg<P>), dim3((unsigned) ls.nseg), dim3(1024), 0, st, ls.segs, tot.as<S>(),
			   fend.as<BUN>(), pre.as<S>(), nxt.as<BUN>(), flags);
	if (whole) {
		hipLaunchKernelGGL((k_rs_bcast_seg<P>), tg, tb, 0, st, p, ls.segs, ls.tiles, tot.as<S>(), pre.as<S>(), out,
				   flags);
	} else {
		hipLaunchKernelGGL((k_rs_write_seg<P>), tg, tb, 0, st, p, o, fwd, ls.segs, ls.tiles, pre.as<S>(),
				   nxt.as<BUN>(), 0, out, flags);
		hipLaunchKernelGGL((k_rs_write_seg<P>), tg, tb, 0, st, p, o, fwd, ls.segs, ls.tiles, pre.as<S>(),
				   nxt.as<BUN>(), 1, out, flags);
	}
	return sync() ? 0 : -1;
}

}  // namespace mgdk
