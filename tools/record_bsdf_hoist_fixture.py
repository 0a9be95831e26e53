#!/usr/bin/env python3
"""Run ON THE GPU BOX, with MIPT_LIBRARY naming a build of the commit BEFORE the per-vertex BSDF terms (variants/libmipt_parent.so): records
tests/golden/bsdf_hoist_queries.npz, the fixture of tests/test_gpu_bsdf_hoist.py -- that file's queries and what pt_debug_bsdf_query of the
named library answers, EVALUATE and SAMPLE, MIS and not.  Both kernel builds (units 0 and 1) must agree with each other before anything
is written; how far the answers are from the CPU oracle's is printed, not required.
usage: MIPT_LIBRARY=$PWD/variants/libmipt_parent.so python tools/record_bsdf_hoist_fixture.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_bsdf_hoist as T                                               # noqa: E402
from gltf_renderer_amd.renderer import Renderer                              # noqa: E402
from oracle import pyoracle                                                   # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
print("library: %s" % (os.environ.get("MIPT_LIBRARY") or "the in-tree build"))
q, u, _ = T.hoist_queries()
pyoracle.build()
r, o = Renderer(), pyoracle.Oracle()
rec = {"q_eval": q, "u": u}
for name, op, flags in T.RUNS:
    qq = q if op == T.EVALUATE else T.sample_queries(q, u)
    g0, g1 = T.gpu_bsdf(r, 0, op, flags, qq), T.gpu_bsdf(r, 1, op, flags, qq)
    assert T.same_bits(g0, g1).all(), (name, "the two builds differ", int((~T.same_bits(g0, g1).all(axis=1)).sum()))
    exact = int((g0.view(np.uint32) != g1.view(np.uint32)).any(axis=1).sum())
    want = o.bsdf_query_many(op, flags, qq)
    bad = ~T.same_bits(g0, want).all(axis=1)
    print("%s: %d queries, units agree (%d rows differ in a NaN's payload only), %d differ from the oracle%s" %
          (name, len(qq), exact, int(bad.sum()), (": first %d" % int(np.flatnonzero(bad)[0])) if bad.any() else ""))
    assert (g0[:, 15] == 0).all() and (op == T.SAMPLE or ((g0[:, 7:9] == 0).all() and T.same_bits(g0[:, 4:7], qq[:, T.ARG]).all()))
    if "lobes" not in rec:
        rec["lobes"] = np.ascontiguousarray(g0[:, 9:15])
    assert T.same_bits(rec["lobes"], g0[:, 9:15]).all(), name
    rec["out_" + name] = T.compact(name, g0)
    assert T.same_bits(T.expand(rec, name, qq), g0).all()
r.close(); o.close()
np.savez_compressed(out_path, **rec)
print("wrote %s: %d bytes" % (out_path, os.path.getsize(out_path)))
