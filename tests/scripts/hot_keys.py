"""Worst cases of the two hash builds (not part of the suite): `python tests/scripts/hot_keys.py`
  A  500 000 copies of ONE triangle                      -> one hot key in the UV-dedup table
  B  500 000 different triangles with identical content  -> one hot key in the digest table (periodic texture, shifts by whole periods)
Prints the phase times; both results are checked against the obvious expectation (1 OMM block)."""
import os, sys, time, ctypes as C
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np, ommtest as ot, bench
lib = ot.Lib("product"); b = lib.create_baker()
import setup_cases
n = 500000
tex, (caseA, caseB) = setup_cases.hot_key_cases(n)
t = lib.create_texture(b, [tex], alpha_cutoff=0.5)
def run(name, uv):
    ix = np.arange(3 * n, dtype=np.uint32)
    d = ot.make_desc(t, uv, ix, 6, addr=ot.WRAP, promo=ot.PROMO_FORCE_OPAQUE)
    for it in range(2):
        t0 = time.time(); r = lib.bake(b, d, want_stats=False); dt = time.time() - t0
    tm = bench.get_timings(lib, b)
    print("%s: %d OMM blocks, %d unique items, bake %.1f ms; setup %.2f triage %.2f classify %.2f digest %.2f tail %.2f gather %.2f" %
          (name, len(r.descs), tm.uniqueItems, dt * 1e3, tm.setupMs, tm.triageMs, tm.classifyMs, tm.digestMs, tm.tailMs, tm.gatherMs))
    return r
rA = run("A (one triangle x 500000)", caseA[1])
assert caseA[2](len(rA.descs)), len(rA.descs)
rB = run("B (500000 shifted copies)", caseB[1])
assert caseB[2](len(rB.descs)), len(rB.descs)   # (nearly) identical content everywhere: a few dozen blocks, 500 000 references
