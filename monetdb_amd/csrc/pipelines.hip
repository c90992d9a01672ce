// pipelines.hip -- the op-at-a-time TPC-H Q1 / Q6 MAL plans composed from
// the device GDK operators, exactly as the reference's MAL interpreter
// calls them (algebra.select x2, thetaselect,
// projection x2, batcalc.*, aggr.sum; §3.3 Q1: thetaselect, projection x6,
// group.group, group.subgroup, batcalc.- + * + *, aggr.subsum x4 (+ disc),
// aggr.subcount, aggr.subavg x3).  Used as the exact fallback of the fused kernels and as
// the "drop-in" timing of the GDK boundary.
#include <cstring>
#include <vector>

#include "mgdk_internal.h"

using namespace mgdk;

namespace {
struct Bats {
	std::vector<mgdk_bat *> v;
	mgdk_bat *add(mgdk_bat *b) { v.push_back(b); return b; }
	~Bats() { for (mgdk_bat *b : v) mgdk_BBPunfix(b); }
};
// the plan's result columns read back with one wait (the result export of
// the MAL plan), through the thread's pinned buffer
struct Readback {
	std::vector<std::pair<const mgdk_bat *, void *>> v;
	void add(const mgdk_bat *b, void *host) { v.emplace_back(b, host); }
	int run()
	{
		size_t tot = 16;
		for (auto &x : v)
			if (x.first->ttype != MGDK_void)
				tot += (x.first->count * (size_t) x.first->twidth + 15) & ~(size_t) 15;
		char *h = (char *) pinned(tot);
		if (h == nullptr)
			return -1;
		size_t o = 0;
		for (auto &x : v) {
			const mgdk_bat *b = x.first;
			const size_t bytes = b->count * (size_t) b->twidth;
			if (b->ttype == MGDK_void || bytes == 0)
				continue;
			if (!hip_ok(hipMemcpyAsync(h + o, b->theap, bytes, hipMemcpyDeviceToHost, stream()), "memcpy"))
				return -1;
			o += (bytes + 15) & ~(size_t) 15;
		}
		if (!sync())
			return -1;
		o = 0;
		for (auto &x : v) {
			const mgdk_bat *b = x.first;
			if (b->ttype == MGDK_void) {
				if (mgdk_BATdownload(b, x.second) < 0)
					return -1;
				continue;
			}
			const size_t bytes = b->count * (size_t) b->twidth;
			memcpy(x.second, h + o, bytes);
			o += (bytes + 15) & ~(size_t) 15;
		}
		return 0;
	}
};
}  // namespace

namespace mgdk {

int
q1_opatatime(mgdk_bat *shipdate, mgdk_bat *rf, mgdk_bat *ls, mgdk_bat *qty, mgdk_bat *price,
	     mgdk_bat *disc, mgdk_bat *tax, int32_t dmax, mgdk_q1row *rows, int maxgroups, int *ngroups)
{
	ProfScope prof("q1_opatatime");
	Bats t;
	mgdk_bat *c1 = t.add(mgdk_BATthetaselect(shipdate, nullptr, &dmax, "<="));
	if (!c1)
		return -1;
	mgdk_bat *prf = t.add(mgdk_BATproject(c1, rf));
	mgdk_bat *pls = t.add(mgdk_BATproject(c1, ls));
	mgdk_bat *pq = t.add(mgdk_BATproject(c1, qty));
	mgdk_bat *pp = t.add(mgdk_BATproject(c1, price));
	mgdk_bat *pd = t.add(mgdk_BATproject(c1, disc));
	mgdk_bat *pt = t.add(mgdk_BATproject(c1, tax));
	if (!prf || !pls || !pq || !pp || !pd || !pt)
		return -1;
	mgdk_bat *g1, *e1, *h1, *g2, *e2, *h2;
	if (mgdk_BATgroup(&g1, &e1, &h1, prf, nullptr, nullptr, nullptr, nullptr) < 0)
		return -1;
	t.add(g1), t.add(e1), t.add(h1);
	if (mgdk_BATgroup(&g2, &e2, &h2, pls, nullptr, g1, e1, h1) < 0)
		return -1;
	t.add(g2), t.add(e2), t.add(h2);
	int64_t hundred = 100;
	mgdk_bat *omd = t.add(mgdk_BATcalccstsub(&hundred, MGDK_lng, pd, nullptr, MGDK_lng));
	mgdk_bat *dp = omd ? t.add(mgdk_BATcalcmul(pp, omd, nullptr, nullptr, MGDK_hge)) : nullptr;
	mgdk_bat *opt = t.add(mgdk_BATcalccstadd(&hundred, MGDK_lng, pt, nullptr, MGDK_lng));
	mgdk_bat *ch = (dp && opt) ? t.add(mgdk_BATcalcmul(dp, opt, nullptr, nullptr, MGDK_hge)) : nullptr;
	if (!ch)
		return -1;
	mgdk_bat *s1 = t.add(mgdk_BATgroupsum(pq, g2, e2, nullptr, MGDK_hge, true));
	mgdk_bat *s2 = t.add(mgdk_BATgroupsum(pp, g2, e2, nullptr, MGDK_hge, true));
	mgdk_bat *s3 = t.add(mgdk_BATgroupsum(dp, g2, e2, nullptr, MGDK_hge, true));
	mgdk_bat *s4 = t.add(mgdk_BATgroupsum(ch, g2, e2, nullptr, MGDK_hge, true));
	mgdk_bat *s5 = t.add(mgdk_BATgroupsum(pd, g2, e2, nullptr, MGDK_hge, true));
	mgdk_bat *cn = t.add(mgdk_BATgroupcount(pq, g2, e2, nullptr, MGDK_lng, false));
	// aggr.subavg (3 outputs) of quantity, extendedprice, discount
	mgdk_bat *av[3], *rm[3], *ac[3];
	mgdk_bat *avin[3] = {pq, pp, pd};
	for (int k = 0; k < 3; k++) {
		if (mgdk_BATgroupavg3(&av[k], &rm[k], &ac[k], avin[k], g2, e2, nullptr, true) < 0)
			return -1;
		t.add(av[k]), t.add(rm[k]), t.add(ac[k]);
	}
	// extents are positions in the projected (filtered) columns
	mgdk_bat *krf = t.add(mgdk_BATproject(e2, prf));
	mgdk_bat *kls = t.add(mgdk_BATproject(e2, pls));
	mgdk_bat *krow = t.add(mgdk_BATproject(e2, c1));   // lineitem oid of each group's first row
	if (!s1 || !s2 || !s3 || !s4 || !s5 || !cn || !krf || !kls || !krow)
		return -1;
	// ORDER BY l_returnflag, l_linestatus: algebra.sort on the first key,
	// the subsort of the second within its groups, every output column
	// projected through the final order (the plan's leftfetchjoins)
	{
		mgdk_bat *sa, *oa, *ga, *sb, *ob, *gb;
		SortInternal no_oidx;   // the plan's sorts of projected temporaries
		if (mgdk_BATsort(&sa, &oa, &ga, krf, nullptr, nullptr, false, false, false) < 0)
			return -1;
		t.add(sa), t.add(oa), t.add(ga);
		if (mgdk_BATsort(&sb, &ob, &gb, kls, oa, ga, false, false, false) < 0)
			return -1;
		t.add(sb), t.add(ob);
		if (gb)
			t.add(gb);
		mgdk_bat **outs[] = {&s1, &s2, &s3, &s4, &s5, &cn, &krf, &kls, &krow,
				     &av[0], &av[1], &av[2], &rm[0], &rm[1], &rm[2]};
		for (mgdk_bat **o : outs)
			if (!(*o = t.add(mgdk_BATproject(ob, *o))))
				return -1;
	}
	const BUN ng = e2->count;
	if ((int) ng > maxgroups) {
		seterr("q1: more groups (%llu) than room for results", (unsigned long long) ng);
		return -1;
	}
	std::vector<hge> v1(ng), v2(ng), v3(ng), v4(ng), v5(ng);
	std::vector<int64_t> vc(ng);
	std::vector<oid> ve(ng);
	std::vector<uint8_t> vr(ng), vl(ng);
	std::vector<int64_t> va[3], vrm[3];
	Readback rb;
	for (int k = 0; k < 3; k++) {
		va[k].resize(ng);
		vrm[k].resize(ng);
		rb.add(av[k], va[k].data());
		rb.add(rm[k], vrm[k].data());
	}
	rb.add(s1, v1.data()), rb.add(s2, v2.data()), rb.add(s3, v3.data()), rb.add(s4, v4.data());
	rb.add(s5, v5.data()), rb.add(cn, vc.data()), rb.add(krow, ve.data()), rb.add(krf, vr.data());
	rb.add(kls, vl.data());
	if (rb.run() < 0)
		return -1;
	for (BUN k = 0; k < ng; k++) {
		mgdk_q1row &r = rows[k];
		memset(&r, 0, sizeof(r));
		r.returnflag = vr[k];
		r.linestatus = vl[k];
		memcpy(r.sum_qty, &v1[k], 16);
		memcpy(r.sum_base_price, &v2[k], 16);
		memcpy(r.sum_disc_price, &v3[k], 16);
		memcpy(r.sum_charge, &v4[k], 16);
		memcpy(r.sum_disc, &v5[k], 16);
		r.count_order = vc[k];
		r.first_row = ve[k];
		r.avg_qty = va[0][k], r.rem_qty = vrm[0][k];
		r.avg_price = va[1][k], r.rem_price = vrm[1][k];
		r.avg_disc = va[2][k], r.rem_disc = vrm[2][k];
	}
	*ngroups = (int) ng;
	return 0;
}

int
q6_opatatime(mgdk_bat *shipdate, mgdk_bat *discount, mgdk_bat *quantity, mgdk_bat *price, int32_t d0,
	     int32_t d1, int64_t dlo, int64_t dhi, int64_t qmax, void *revenue)
{
	Bats t;
	mgdk_bat *c1 = t.add(mgdk_BATselect(shipdate, nullptr, &d0, &d1, true, false, false, false));
	mgdk_bat *c2 = c1 ? t.add(mgdk_BATselect(discount, c1, &dlo, &dhi, true, true, false, false)) : nullptr;
	mgdk_bat *c3 = c2 ? t.add(mgdk_BATthetaselect(quantity, c2, &qmax, "<")) : nullptr;
	mgdk_bat *p1 = c3 ? t.add(mgdk_BATproject(c3, price)) : nullptr;
	mgdk_bat *p2 = c3 ? t.add(mgdk_BATproject(c3, discount)) : nullptr;
	mgdk_bat *m = (p1 && p2) ? t.add(mgdk_BATcalcmul(p1, p2, nullptr, nullptr, MGDK_hge)) : nullptr;
	if (!m)
		return -1;
	if (m->count == 0) {
		memset(revenue, 0, 16);
		return 0;
	}
	return mgdk_BATsum(revenue, MGDK_hge, m, nullptr, true, true);
}

// the select cascade + sums fragment (mgdk_select_sum_fused) through the
// operators: selects chained through their candidate lists, one projection
// per operand, batcalc.* into hge, aggr.sum
int
select_sum_opatatime(const mgdk_selpred *preds, int npreds, mgdk_bat *s, const mgdk_sumexpr *sums, int nsums,
		     void *results, uint64_t *count)
{
	Bats t;
	mgdk_bat *c = s;
	for (int i = 0; i < npreds; i++) {
		const mgdk_selpred &p = preds[i];
		c = t.add(p.op ? mgdk_BATthetaselect(p.b, c, p.tl, p.op)
			       : mgdk_BATselect(p.b, c, p.tl, p.th, p.li, p.hi, p.anti, p.nil_matches));
		if (!c)
			return -1;
	}
	if (c == nullptr) {
		seterr("select_sum: a predicate or a candidate list is required");
		return -1;
	}
	if (count)
		*count = c->count;
	for (int j = 0; j < nsums; j++) {
		if (sums[j].a == nullptr) {
			seterr("select_sum: a sum needs its first operand");
			return -1;
		}
		mgdk_bat *v = t.add(mgdk_BATproject(c, sums[j].a));
		if (v && sums[j].b) {
			mgdk_bat *pb = t.add(mgdk_BATproject(c, sums[j].b));
			v = pb ? t.add(mgdk_BATcalcmul(v, pb, nullptr, nullptr, MGDK_hge)) : nullptr;
		}
		if (!v)
			return -1;
		if (mgdk_BATsum((char *) results + 16 * (size_t) j, MGDK_hge, v, nullptr, true, true) < 0)
			return -1;
	}
	return 0;
}

// the grouped fragment (mgdk_select_groupsum_fused) through the operators:
// the selects, a projection per key and per factor, BATgroup refined by the
// second key, the constant +- column factors into lng, the products into hge
// from the left, BATgroupsum per sum (and BATgroupcount of the non-nil terms),
// BATgroupcount, and the keys and first rows through the extents.  G is
// mgdk_gsgroup (the keys' bytes) or mgdk_gsgroupw (the hashed entry's twin:
// the keys read back at their own width, sign-extended, str offsets
// zero-extended).  vias (mgdk_select_groupsum_star_opatatime): a column whose
// descriptor is some vias[i].col belongs to a dimension table and is reached
// through the join index V = vias[i].via: two projections where a fact column
// takes one, and a predicate on it selects on the gathered values without a
// candidate list and takes its result through the previous candidate list
template <typename G>
int
select_groupsum_opatatime(const mgdk_selpred *preds, int npreds, mgdk_bat *s, mgdk_bat *const *keys, int nkeys,
			  const mgdk_gsumexpr *sums, int nsums, int maxgroups, int *ngroups, G *groups,
			  void *sumres, uint64_t *nonnil, const mgdk_starvia *vias = nullptr, int nvias = 0)
{
	constexpr bool WIDE = sizeof(((G *) nullptr)->key[0]) == 8;
	if (keys == nullptr || nkeys < 1 || nkeys > 2 || keys[0] == nullptr || ngroups == nullptr || npreds < 0 ||
	    nsums < 0) {
		seterr("select_groupsum: one or two key columns are required");
		return -1;
	}
	if (nvias < 0 || (nvias > 0 && vias == nullptr)) {
		seterr("select_groupsum: the join indexes are missing");
		return -1;
	}
	for (int i = 0; i < nvias; i++)
		if (vias[i].col == nullptr || vias[i].via == nullptr) {
			seterr("select_groupsum: a join index names a dimension column and an oid column");
			return -1;
		}
	Bats t;
	auto via_of = [&](const mgdk_bat *b) -> mgdk_bat * {
		for (int i = 0; i < nvias; i++)
			if (vias[i].col == b)
				return vias[i].via;
		return nullptr;
	};
	// x(c, b): b's values at the candidates c
	auto project = [&](mgdk_bat *c, mgdk_bat *b) -> mgdk_bat * {
		mgdk_bat *v = via_of(b);
		if (v == nullptr)
			return t.add(mgdk_BATproject(c, b));
		mgdk_bat *o = t.add(mgdk_BATproject(c, v));
		return o ? t.add(mgdk_BATproject(o, b)) : nullptr;
	};
	mgdk_bat *c = s;
	for (int i = 0; i < npreds; i++) {
		const mgdk_selpred &p = preds[i];
		mgdk_bat *v = p.b ? via_of(p.b) : nullptr, *b = p.b, *cand = c;
		if (v) {
			// BATproject keeps its left operand's head: without a
			// candidate list the selected oids are the fact table's
			b = c ? project(c, p.b) : t.add(mgdk_BATproject(v, p.b));
			cand = nullptr;
			if (!b)
				return -1;
		}
		mgdk_bat *r = t.add(p.op ? mgdk_BATthetaselect(b, cand, p.tl, p.op)
					 : mgdk_BATselect(b, cand, p.tl, p.th, p.li, p.hi, p.anti, p.nil_matches));
		if (r && v && c)
			r = t.add(mgdk_BATproject(r, c));
		if (!(c = r))
			return -1;
	}
	if (c == nullptr) {
		// no select at all: every row of the keys
		Cand ci;
		mgdk_bat *v = via_of(keys[0]);
		if (cand_init(&ci, v ? v : keys[0], nullptr) < 0 || !(c = t.add(cand_slice(ci))))
			return -1;
	}
	mgdk_bat *g = nullptr, *e = nullptr, *h = nullptr, *k[2] = {nullptr, nullptr};
	for (int j = 0; j < nkeys; j++) {
		if (keys[j] == nullptr)
			return -1;
		// the group struct holds a key of one byte (of 1, 2, 4 or 8 bytes
		// for mgdk_gsgroupw): nothing wider, and no void key, is read back
		auto fits = [](int kw) { return WIDE ? (kw == 1 || kw == 2 || kw == 4 || kw == 8) : kw == 1; };
		if (!fits(keys[j]->twidth)) {
			seterr("select_groupsum: a key column of width %d does not fit the result's keys", (int) keys[j]->twidth);
			return -1;
		}
		if (!(k[j] = project(c, keys[j])))
			return -1;
		if (k[j]->count != 0 && !fits(k[j]->twidth)) {
			seterr("select_groupsum: a key column of width %d does not fit the result's keys", (int) k[j]->twidth);
			return -1;
		}
		mgdk_bat *g2, *e2, *h2;
		if (mgdk_BATgroup(&g2, &e2, &h2, k[j], nullptr, g, e, h) < 0)
			return -1;
		g = t.add(g2), e = t.add(e2), h = t.add(h2);
	}
	const BUN ng = e->count;
	if (ng > (BUN) (maxgroups < 0 ? 0 : maxgroups)) {
		seterr("select_groupsum: more groups (%llu) than room for results", (unsigned long long) ng);
		return -1;
	}
	std::vector<mgdk_bat *> sv(nsums), nv(nsums);
	for (int j = 0; j < nsums; j++) {
		if (sums[j].nf < 1 || sums[j].nf > 3) {
			seterr("select_groupsum: a sum has one to three factors");
			return -1;
		}
		mgdk_bat *x = nullptr;
		for (int q = 0; q < sums[j].nf; q++) {
			const mgdk_gsfactor &f = sums[j].f[q];
			mgdk_bat *v = f.b ? project(c, f.b) : nullptr;
			if (v && f.op == '+')
				v = t.add(mgdk_BATcalccstadd(&f.cst, MGDK_lng, v, nullptr, MGDK_lng));
			else if (v && f.op == '-')
				v = t.add(mgdk_BATcalccstsub(&f.cst, MGDK_lng, v, nullptr, MGDK_lng));
			else if (v && f.op != 0) {
				seterr("select_groupsum: a factor is b, cst + b or cst - b");
				return -1;
			}
			if (v && q > 0)
				v = t.add(mgdk_BATcalcmul(x, v, nullptr, nullptr, MGDK_hge));
			if (!(x = v))
				return -1;
		}
		sv[j] = t.add(mgdk_BATgroupsum(x, g, e, nullptr, MGDK_hge, true));
		nv[j] = t.add(mgdk_BATgroupcount(x, g, e, nullptr, MGDK_lng, true));
		if (!sv[j] || !nv[j])
			return -1;
	}
	mgdk_bat *cn = t.add(mgdk_BATgroupcount(k[0], g, e, nullptr, MGDK_lng, false));
	mgdk_bat *kf = t.add(mgdk_BATproject(e, c));
	mgdk_bat *kk[2] = {t.add(mgdk_BATproject(e, k[0])), nkeys > 1 ? t.add(mgdk_BATproject(e, k[1])) : nullptr};
	if (!cn || !kf || !kk[0] || (nkeys > 1 && !kk[1]))
		return -1;
	std::vector<hge> vs((size_t) ng * nsums);
	std::vector<int64_t> vn((size_t) ng * nsums), vc(ng);
	std::vector<oid> vf(ng);
	std::vector<uint8_t> vk[2] = {std::vector<uint8_t>(WIDE ? ng * 8 : ng), std::vector<uint8_t>(WIDE ? ng * 8 : ng)};
	Readback rb;
	for (int j = 0; j < nsums; j++) {
		rb.add(sv[j], vs.data() + (size_t) j * ng);
		rb.add(nv[j], vn.data() + (size_t) j * ng);
	}
	rb.add(cn, vc.data()), rb.add(kf, vf.data()), rb.add(kk[0], vk[0].data());
	if (nkeys > 1)
		rb.add(kk[1], vk[1].data());
	if (rb.run() < 0)
		return -1;
	for (BUN i = 0; i < ng; i++) {
		G &o = groups[i];
		memset(&o, 0, sizeof(o));
		o.first = vf[i];
		o.count = (uint64_t) vc[i];
		if constexpr (WIDE) {
			for (int j = 0; j < nkeys; j++) {
				const int w = kk[j]->twidth;
				uint64_t v = 0;
				memcpy(&v, vk[j].data() + (size_t) i * w, w);
				const int sh = 64 - 8 * w;
				o.key[j] = kk[j]->ttype == MGDK_str ? (int64_t) v : (int64_t) (v << sh) >> sh;
			}
		} else {
			o.key[0] = vk[0][i];
			o.key[1] = nkeys > 1 ? vk[1][i] : 0;
		}
		for (int j = 0; j < nsums; j++) {
			memcpy((char *) sumres + 16 * ((size_t) i * nsums + j), &vs[(size_t) j * ng + i], 16);
			nonnil[(size_t) i * nsums + j] = (uint64_t) vn[(size_t) j * ng + i];
		}
	}
	*ngroups = (int) ng;
	return 0;
}

}  // namespace mgdk

extern "C" {

int mgdk_select_groupsum_opatatime(const mgdk_selpred *preds, int npreds, mgdk_bat *s, mgdk_bat *const *keys,
				   int nkeys, const mgdk_gsumexpr *sums, int nsums, int maxgroups, int *ngroups,
				   mgdk_gsgroup *groups, void *sumres, uint64_t *nonnil)
{
	return select_groupsum_opatatime(preds, npreds, s, keys, nkeys, sums, nsums, maxgroups, ngroups, groups, sumres,
					 nonnil);
}

int mgdk_select_groupsum_hash_opatatime(const mgdk_selpred *preds, int npreds, mgdk_bat *s, mgdk_bat *const *keys,
					int nkeys, const mgdk_gsumexpr *sums, int nsums, int maxgroups, int *ngroups,
					mgdk_gsgroupw *groups, void *sumres, uint64_t *nonnil)
{
	return select_groupsum_opatatime(preds, npreds, s, keys, nkeys, sums, nsums, maxgroups, ngroups, groups, sumres,
					 nonnil);
}

int mgdk_select_groupsum_star_opatatime(const mgdk_selpred *preds, int npreds, mgdk_bat *s, mgdk_bat *const *keys,
					int nkeys, const mgdk_gsumexpr *sums, int nsums, const mgdk_starvia *vias,
					int nvias, int maxgroups, int *ngroups, mgdk_gsgroupw *groups, void *sumres,
					uint64_t *nonnil)
{
	return select_groupsum_opatatime(preds, npreds, s, keys, nkeys, sums, nsums, maxgroups, ngroups, groups, sumres,
					 nonnil, vias, nvias);
}

int mgdk_select_sum_opatatime(const mgdk_selpred *preds, int npreds, mgdk_bat *s, const mgdk_sumexpr *sums,
			      int nsums, void *results, uint64_t *count)
{
	return select_sum_opatatime(preds, npreds, s, sums, nsums, results, count);
}

// op-at-a-time variants exported for timing the GDK-boundary path
int mgdk_q6_opatatime(mgdk_bat *shipdate, mgdk_bat *discount, mgdk_bat *quantity, mgdk_bat *price,
		      int32_t d0, int32_t d1, int64_t dlo, int64_t dhi, int64_t qmax, void *revenue)
{
	return q6_opatatime(shipdate, discount, quantity, price, d0, d1, dlo, dhi, qmax, revenue);
}

int mgdk_q1_opatatime(mgdk_bat *shipdate, mgdk_bat *rf, mgdk_bat *ls, mgdk_bat *qty, mgdk_bat *price,
		      mgdk_bat *disc, mgdk_bat *tax, int32_t dmax, mgdk_q1row *rows, int maxgroups, int *ngroups)
{
	return q1_opatatime(shipdate, rf, ls, qty, price, disc, tax, dmax, rows, maxgroups, ngroups);
}

}  // extern "C"
