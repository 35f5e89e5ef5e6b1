"""Replays ONE case of tests/stress_sweeps.py (its `case=` number) and prints, family by family, whether it matches the oracle and
which entries differ.
   python tests/sweep_case.py 499794305 [KEY=VALUE ...]     (extra environment knobs override the case's; KEY= removes one)"""
import os
import sys

os.environ["GENPHI_ENV_HOOKS"] = "1"      # environment hooks are read by the library only under this gate
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stress_sweeps as S


def main():
    import genlib_jl_amd as gen
    case = int(sys.argv[1])
    make = S.make_case
    overrides = dict(kv.split("=", 1) for kv in sys.argv[2:])

    def make_with_overrides(k):
        c = make(k)
        for key, v in overrides.items():
            if v == "":
                c["env"].pop(key, None)
            else:
                c["env"][key] = v
        return c

    S.make_case = make_with_overrides
    print("case", case, S.describe(S.make_case(case)))
    what, _ = S.run_case(case, gen, report=print)
    print("differs:", what if what else "nothing")
    return 1 if what else 0


if __name__ == "__main__":
    sys.exit(main())
