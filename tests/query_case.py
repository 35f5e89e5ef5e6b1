"""Replays ONE case of tests/stress_queries.py (its `case=` number) and prints the plan (last-step mode, whether the proband cut stayed in
place, the sparse cut), then state by state and query by query whether the device agrees with the oracle.
   python tests/query_case.py 499794305 [KEY=VALUE ...]     (extra tuning knobs override the case's; KEY= removes one)"""
import os
import sys

os.environ["GENPHI_ENV_HOOKS"] = "1"      # environment hooks are read by the library only under this gate
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stress_queries as S


def main():
    import genlib_jl_amd as gen
    from oracle import oracle as O
    O.fit_threads_to_quota()
    case = int(sys.argv[1])
    overrides = dict(kv.split("=", 1) for kv in sys.argv[2:])

    def make_with_overrides(k):
        c = S.make_case(k)
        for key, v in overrides.items():
            if v == "":
                c["tuning"].pop(key, None)
            else:
                c["tuning"][key] = v
        return c

    print("case", case, S.describe(make_with_overrides(case)))
    what, _ = S.run_case(case, gen, O, report=print, make=make_with_overrides)
    print("differs:", what if what else "nothing")
    return 1 if what else 0


if __name__ == "__main__":
    sys.exit(main())
