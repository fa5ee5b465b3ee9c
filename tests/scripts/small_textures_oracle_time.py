"""The oracle alone, on the CPU, over the whole case list of test_small_textures_gpu.py: it must accept every bake, and no case may cost it more
than a couple of seconds.  Prints the time of each case and the total (the figure in tests/README.md).  No GPU, no product library.

    python tests/scripts/small_textures_oracle_time.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ommtest as ot                   # noqa: E402
import small_texture_cases as stc      # noqa: E402


def oracle_only(product, oracle, mips, uv, ix, level, sat=True, zorder=False, cutoff=0.5, expect=ot.SUCCESS, knobs=(), **kw):
    b = oracle.create_baker()
    t = oracle.create_texture(b, mips, alpha_cutoff=cutoff if sat else -1.0, disable_zorder=zorder)
    d = ot.make_desc(t, uv, ix, level, alpha_cutoff=cutoff, **kw)
    r = oracle.bake(b, d, expect=expect)
    oracle.destroy_texture(b, t)
    oracle.destroy_baker(b)
    return r


def main():
    orc = ot.Lib("oracle")
    total, worst, bakes = 0.0, (0.0, None), 0
    for case in stc.cases():
        t0 = time.time()
        stc.run_case(oracle_only, None, orc, case)
        dt = time.time() - t0
        bakes += len(stc.bakes_of(case[1], *case[2]))
        total += dt
        worst = max(worst, (dt, case[0]))
        print("%-24s %6.2f s" % (case[0], dt), flush=True)
    for case in stc.chain_cases():
        t0 = time.time()
        stc.run_chain_case(oracle_only, None, orc, case)
        dt = time.time() - t0
        bakes += 4
        total += dt
        worst = max(worst, (dt, case[0]))
        print("%-24s %6.2f s" % (case[0], dt), flush=True)
    print("total %.1f s over %d bakes, slowest case %s %.2f s" % (total, bakes, worst[1], worst[0]))


if __name__ == "__main__":
    main()
