"""Wall time of the fused Q6's first call on fresh columns (it builds the
column images it asks for) against the calls after it."""
import os
import sys
import time

sys.path.insert(0, ".")
from monetdb_amd import gdk

gdk.init(0)
rows = int(os.environ.get("Q6_ROWS", "600121500"))
mk = lambda y, m, d: (((y + 4712) * 12 + m - 1) << 5) | d
variants = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [28, 26, 24, 19]
# every kernel of every variant, image builds included, runs once on small
# columns first: the first calls timed below pay no code loading
for variant in variants:
    warm = gdk.tpch_lineitem(3, 0, 1 << 21, 20_000)
    gdk.q6_set_variant(variant, 64)
    gdk.q6_fused(warm["shipdate"], warm["discount"], warm["quantity"], warm["extendedprice"],
                 mk(1994, 1, 1), mk(1995, 1, 1), 5, 7, 2400)
    del warm
for variant in variants:
    cols = gdk.tpch_lineitem(20241024, 0, rows, max(1, rows // 30))
    args = (cols["shipdate"], cols["discount"], cols["quantity"], cols["extendedprice"],
            mk(1994, 1, 1), mk(1995, 1, 1), 5, 7, 2400)
    gdk.q6_set_variant(variant, 128 if variant < 24 else 64)
    gdk.sync()
    ms = []
    for _ in range(6):
        t = time.perf_counter()
        rev = gdk.q6_fused(*args)
        ms.append((time.perf_counter() - t) * 1e3)
    images = [gdk.colimg_info(cols[k])[:2] for k in ("shipdate", "discount", "quantity")]
    packs = [gdk.colpack_info(cols[k]) for k in ("shipdate", "discount", "quantity")]
    print("variant %d: first call %.3f ms, next calls %s ms, images (state, width) %s, packed images "
          "(state, bits, base, stride) %s, revenue %d, bytes %d" % (
              variant, ms[0], " ".join("%.3f" % x for x in ms[1:]), images, packs, rev, gdk.q6_last_bytes()))
    del cols, args
    gdk.lib().mgdk_mem_release_cache()
