"""One-off stress of the single-pass scans and the sort path of the tail at counts the suite does not run (the counts to 32 769, on every tile, chunk and
path edge, are family P of tests/test_tail_gpu.py): the same generator and the same checks -- HIP library vs oracle on full arrays, and the library's
result against the numpy restatement of tests/tail_cases.py -- plus test_descriptor_order_and_offsets_both_tail_paths at those counts.
usage (GPU box): python tests/scripts/stress_tail_paths.py"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

COUNTS = (65537, 131072, 250001)


def main():
    import ommtest as ot
    import tail_cases as tc
    import test_gpu_parity as tg
    product, oracle = ot.Lib("product"), ot.Lib("oracle")
    flags_list = [ot.FLAG_THREADS, ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL, ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL | ot.FLAG_NO_DEDUP | ot.FLAG_FORCE32, ot.FLAG_THREADS | ot.FLAG_NO_DEDUP]
    n = 0
    for count in COUNTS:
        for fmt in tc.FORMATS:
            for mode in tc.LEVEL_MODES:
                case = tc.p_all_case(count, mode, fmt)
                raw = tc.bake(oracle, case, flags=tc.RAW_FLAGS)
                r = tg.both(product, oracle, [case["tex"]], case["uv"], case["ix"], case["gmax"], **tc.desc_kw(case))
                tc.check_result(case, r, tc.restate_tail(tc.tail_inputs(case, raw), case["flags"]))
                n += 1
                print("ok", case["name"], flush=True)
        for flags in flags_list:
            tg.test_descriptor_order_and_offsets_both_tail_paths(product, oracle, count, flags)
            n += 1
            print("ok", count, hex(flags), flush=True)
    print("stress ok:", n, "cases")


if __name__ == "__main__":
    main()
