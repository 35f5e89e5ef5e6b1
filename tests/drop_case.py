"""Replays ONE case of tests/stress_drops.py (its `case=` number) and prints, family by family, whether it matches the reference and
the first entries that differ.
   python tests/drop_case.py 499794305 [KEY=VALUE ...]
KEY: seed, sort, api (handles / wrappers), fresh_seed, or family.key of a family's own dict (simu.S, simu.panel, simu.no_sample,
ident.S, ident.panel_cols, ident.labels, ident.all_pairs, link.L, link.q, link.S, link.panel_sims, link.labels, link.all_pairs);
VALUE: an integer (0x.. too), True or False, or a word."""
import os
import sys

os.environ["GENPHI_ENV_HOOKS"] = "1"      # environment hooks are read by the library only under this gate
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stress_drops as D


def _value(v):
    if v in ("True", "False"):
        return v == "True"
    try:
        return int(v, 0)
    except ValueError:
        return v


def main():
    import genlib_jl_amd as gen
    case = int(sys.argv[1])
    make = D.make_case
    overrides = dict(kv.split("=", 1) for kv in sys.argv[2:])

    def make_with_overrides(k):
        c = make(k)
        for key, v in overrides.items():
            fam, _, name = key.rpartition(".")
            d = c[fam] if fam else c
            if name not in d:
                raise KeyError("%s is no key of a case (see the head of tests/drop_case.py)" % key)
            d[name] = _value(v)
        return c

    D.make_case = make_with_overrides
    c = D.make_case(case)
    print("case", case, D.describe(c))
    ped = D.genealogy(c, gen)
    args = (ped.ind, ped.father, ped.mother)
    refs = D.references(c, args)
    hs = D.handles(c, gen, args)
    print("classes:", ", ".join(sorted(D.classes(c, *hs, *refs))))
    for h in hs:
        h.close()
    what, _ = D.run_case(case, gen, report=print)
    print("differs:", what if what else "nothing")
    return 1 if what else 0


if __name__ == "__main__":
    sys.exit(main())
