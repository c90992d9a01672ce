// selnorm.h -- the argument normalisation of BATselect / BATthetaselect,
// shared by the operators (select.hip) and the fused select-cascade sums
// (selectsum.hip): every request is reduced to an empty result, all
// candidates, or one closed predicate for the scan
// (gdk/gdk_select.c:1342-1564, nil/anti table :1288-1340; scanfunc :300-446).
#pragma once

#include <cmath>
#include <cstring>
#include <limits>

#include "mgdk_internal.h"

namespace mgdk {

enum SelMode { SEL_RANGE = 0, SEL_ANTI = 1, SEL_EQ = 2, SEL_EQNIL = 3, SEL_NOTNIL = 4 };

template <typename T>
struct SelPred {
	int mode;
	bool nil_matches;
	T vl, vh;
};

template <typename T> struct Lim {
	static T minv() { return std::numeric_limits<T>::min() + 1; }   // GDK_T_min = nil + 1
	static T maxv() { return std::numeric_limits<T>::max(); }
	static T prev(T x) { return x - 1; }
	static T next(T x) { return x + 1; }
	static bool isnil(T x) { return x == std::numeric_limits<T>::min(); }
	static T nil() { return std::numeric_limits<T>::min(); }
};
template <> struct Lim<uint64_t> {   // oid: nil = 1<<63, GDK_oid_min = 0, max = 2^63-1
	static uint64_t minv() { return 0; }
	static uint64_t maxv() { return ((uint64_t) 1 << 63) - 1; }
	static uint64_t prev(uint64_t x) { return x - 1; }
	static uint64_t next(uint64_t x) { return x + 1; }
	static bool isnil(uint64_t x) { return x == ((uint64_t) 1 << 63); }
	static uint64_t nil() { return (uint64_t) 1 << 63; }
};
template <> struct Lim<hge> {
	static hge maxv() { return (hge) (((uhge) 1 << 127) - 1); }
	static hge minv() { return -maxv(); }
	static hge prev(hge x) { return x - 1; }
	static hge next(hge x) { return x + 1; }
	static bool isnil(hge x) { return x == (hge) ((uhge) 1 << 127); }
	static hge nil() { return (hge) ((uhge) 1 << 127); }
};
template <> struct Lim<float> {
	static float minv() { return -std::numeric_limits<float>::max(); }
	static float maxv() { return std::numeric_limits<float>::max(); }
	static float prev(float x) { return nextafterf(x, -std::numeric_limits<float>::max()); }
	static float next(float x) { return nextafterf(x, std::numeric_limits<float>::max()); }
	static bool isnil(float x) { return std::isnan(x); }
	static float nil() { return std::numeric_limits<float>::quiet_NaN(); }
};
template <> struct Lim<double> {
	static double minv() { return -std::numeric_limits<double>::max(); }
	static double maxv() { return std::numeric_limits<double>::max(); }
	static double prev(double x) { return nextafter(x, -std::numeric_limits<double>::max()); }
	static double next(double x) { return nextafter(x, std::numeric_limits<double>::max()); }
	static bool isnil(double x) { return std::isnan(x); }
	static double nil() { return std::numeric_limits<double>::quiet_NaN(); }
};

template <typename T>
static int
cmp3(T a, T b)
{
	// ATOMcmp: nil smallest and equal to itself
	bool an = Lim<T>::isnil(a), bn = Lim<T>::isnil(b);
	if (an || bn)
		return an && bn ? 0 : an ? -1 : 1;
	return (a > b) - (a < b);
}

// outcome of the normalisation: no candidate qualifies, every candidate
// does, or the candidates satisfying *p do
enum SelOutcome { SELN_EMPTY, SELN_ALL, SELN_SCAN };

// The body of BATselect after candidate setup, for value type T, up to the
// scan: tnonil is the column's "holds no nil" property.
template <typename T>
static SelOutcome
sel_normalise(bool tnonil, const T *tlp, const T *thp, bool li, bool hi, bool anti, bool nil_matches, SelPred<T> *p)
{
	const T nil = Lim<T>::nil();
	T tl = *tlp, th = thp ? *thp : T{};
	bool th_null = thp == nullptr;
	bool lnil = cmp3(tl, nil) == 0;
	bool lval = !lnil || th_null;
	bool equi = th_null || (lval && cmp3(tl, th) == 0);
	bool hval;
	if (lnil && nil_matches && (th_null || cmp3(th, nil) == 0)) {
		equi = true;
		lval = true;
	}
	if (equi) {
		if (th_null)
			hi = li;
		th = tl;
		hval = true;
		if (!anti && (!li || !hi))
			return SELN_EMPTY;
	} else {
		nil_matches = false;
		hval = cmp3(th, nil) != 0;
	}
	if (anti) {
		if (lval != hval) {
			bool ti = li;
			li = !hi;
			hi = !ti;
			T tv = tl;
			tl = th;
			th = tv;
			ti = lval;
			lval = hval;
			hval = ti;
			lnil = cmp3(tl, nil) == 0;
			anti = false;
		} else if (!lval && !hval) {
			return SELN_EMPTY;
		} else if ((equi && (lnil || !(li && hi))) || cmp3(tl, th) > 0) {
			if (equi && !lnil && nil_matches && !(li && hi))
				return SELN_ALL;
			*p = SelPred<T>{SEL_NOTNIL, false, tl, th};
			if (tnonil)
				return SELN_ALL;
			return SELN_SCAN;
		} else {
			equi = false;   // anti-equi handled by the scan (gdk_select.c:1519)
		}
	}
	if (hval && (equi ? !li || !hi : cmp3(tl, th) > 0))
		return SELN_EMPTY;
	if (equi && lnil && tnonil)
		return SELN_EMPTY;
	if (!equi && !lval && !hval && lnil && tnonil)
		return SELN_ALL;

	// scanfunc normalisation (gdk_select.c:300-446)
	T vl = tl, vh = th;
	if (anti && li) {
		if (vl == Lim<T>::minv()) {
			anti = false;
			vl = vh;
			li = !hi;
			hval = false;
		} else {
			vl = Lim<T>::prev(vl);
			li = false;
		}
	}
	if (anti && hi) {
		if (vh == Lim<T>::maxv()) {
			anti = false;
			vh = vl;
			hi = !li;
			lval = false;
		} else {
			vh = Lim<T>::next(vh);
			hi = false;
		}
	}
	if (!anti) {
		if (lval) {
			if (!li) {
				if (vl == Lim<T>::maxv())
					return SELN_EMPTY;
				vl = Lim<T>::next(vl);
				li = true;
			}
		} else {
			vl = Lim<T>::minv();
			li = true;
			lval = true;
		}
		if (hval) {
			if (!hi) {
				if (vh == Lim<T>::minv())
					return SELN_EMPTY;
				vh = Lim<T>::prev(vh);
				hi = true;
			}
		} else {
			vh = Lim<T>::maxv();
			hi = true;
			hval = true;
		}
		if (vl > vh)
			return SELN_EMPTY;
	}
	p->vl = vl;
	p->vh = vh;
	p->nil_matches = nil_matches;
	if (equi)
		p->mode = lnil ? SEL_EQNIL : SEL_EQ;
	else if (anti)
		p->mode = SEL_ANTI;
	else
		p->mode = SEL_RANGE;
	return SELN_SCAN;
}

// BATthetaselect's mapping onto BATselect (gdk/gdk_select.c:2103-2154) for a
// column of base type bt: the arguments of the BATselect call that answers
// (b, val, op); tl / th may point into nilv, so the struct is used in place
struct ThetaArgs {
	alignas(16) unsigned char nilv[16];
	const void *tl, *th;
	bool li, hi, anti, nil_matches;
};
// 0: call BATselect with *a; 1: val is nil, the result is empty; -1: the
// type has no device path; -2: unknown operator (the caller sets the error)
static inline int
theta_args(int bt, const void *val, const char *op, ThetaArgs *a)
{
	auto set = [a](const void *tl, const void *th, bool li, bool hi, bool anti, bool nil_matches) {
		a->tl = tl;
		a->th = th;
		a->li = li;
		a->hi = hi;
		a->anti = anti;
		a->nil_matches = nil_matches;
		return 0;
	};
	if (strcmp(op, "eq") == 0)
		return set(val, nullptr, true, true, false, true);
	if (strcmp(op, "ne") == 0)
		return set(val, nullptr, true, true, true, true);
	unsigned char *nilv = a->nilv;
	bool isnil = false;
	switch (bt) {
	case MGDK_str:
		nilv[0] = 0x80;
		nilv[1] = 0;
		isnil = ((const unsigned char *) val)[0] == 0x80 && ((const unsigned char *) val)[1] == 0;
		break;
	case MGDK_bte: *(int8_t *) nilv = INT8_MIN; isnil = *(const int8_t *) val == INT8_MIN; break;
	case MGDK_sht: *(int16_t *) nilv = INT16_MIN; isnil = *(const int16_t *) val == INT16_MIN; break;
	case MGDK_int: *(int32_t *) nilv = INT32_MIN; isnil = *(const int32_t *) val == INT32_MIN; break;
	case MGDK_lng: *(int64_t *) nilv = INT64_MIN; isnil = *(const int64_t *) val == INT64_MIN; break;
	case MGDK_void:
	case MGDK_oid: *(uint64_t *) nilv = MGDK_OID_NIL; isnil = *(const uint64_t *) val == MGDK_OID_NIL; break;
	case MGDK_hge: {
		hge n = (hge) ((uhge) 1 << 127);
		memcpy(nilv, &n, 16);
		isnil = memcmp(val, &n, 16) == 0;
		break;
	}
	case MGDK_flt: *(float *) nilv = std::numeric_limits<float>::quiet_NaN(); isnil = std::isnan(*(const float *) val); break;
	case MGDK_dbl: *(double *) nilv = std::numeric_limits<double>::quiet_NaN(); isnil = std::isnan(*(const double *) val); break;
	default:
		return -1;
	}
	if (isnil)
		return 1;
	if (op[0] == '=' && ((op[1] == '=' && op[2] == 0) || op[1] == 0))
		return set(val, nullptr, true, true, false, false);
	if (op[0] == '!' && op[1] == '=' && op[2] == 0)
		return set(val, nullptr, true, true, true, false);
	if (op[0] == '<') {
		if (op[1] == 0)
			return set(nilv, val, false, false, false, false);
		if (op[1] == '=' && op[2] == 0)
			return set(nilv, val, false, true, false, false);
		if (op[1] == '>' && op[2] == 0)
			return set(val, nullptr, true, true, true, false);
	}
	if (op[0] == '>') {
		if (op[1] == 0)
			return set(val, nilv, false, false, false, false);
		if (op[1] == '=' && op[2] == 0)
			return set(val, nilv, true, false, false, false);
	}
	return -2;
}

}  // namespace mgdk
