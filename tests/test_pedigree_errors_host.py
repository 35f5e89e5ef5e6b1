"""Which error a malformed pedigree gets is behaviour: gen.simu, gen.simuIdentity and gen.implex index the pedigree through
csrc/pedigree_index.cpp (the first offending row decides; within a row the duplicate, then the father, then the mother; then the
probands), and callers see the return code and the text of genphi_last_error().  Every case below goes through the three create
functions -- host only, no GPU -- with small dense IDs (the direct table of Ranks) and with the same IDs spread out and partly
negative (its hash map: the table keeps the LAST rank of a duplicated ID, the map the FIRST, so the row that reports it differs).

The expected (code, text) pairs are tests/golden/pedigree_errors.json, recorded with record() below from the library of the commit
named in that file, BEFORE the three plans shared their index:
    python tests/test_pedigree_errors_host.py ROOT_OF_A_BUILT_CHECKOUT COMMIT > tests/golden/pedigree_errors.json"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pedigree_errors.json")

# name: (ind, father, mother, probands); 0 = unknown parent, 99 = an ID that is nowhere
CASES = {
    "valid": ([1, 2, 3, 4], [0, 0, 1, 3], [0, 0, 2, 2], [4, 3]),
    "duplicate alone": ([1, 2, 2, 3], [0, 0, 0, 1], [0, 0, 0, 2], [3]),
    "father late": ([1, 2, 3], [0, 3, 0], [0, 0, 0], [2]),
    "mother late": ([1, 2, 3], [0, 0, 0], [0, 3, 0], [2]),
    "unknown father": ([1, 2, 3], [0, 99, 0], [0, 1, 0], [2]),
    "unknown mother": ([1, 2, 3], [0, 1, 0], [0, 99, 0], [2]),
    "father late and mother unknown in one row": ([1, 2, 3], [0, 3, 0], [0, 99, 0], [2]),
    "own parent": ([1, 2, 3], [0, 2, 0], [0, 0, 0], [3]),
    "duplicate and late parent in the same rows": ([1, 2, 2, 4], [0, 4, 4, 0], [0, 0, 0, 0], [1]),
    "late parent in a row before the duplicate": ([1, 5, 2, 2, 6], [0, 6, 0, 0, 0], [0, 0, 0, 0, 0], [1]),
    "late parent in a row after the duplicate": ([1, 2, 2, 5, 6], [0, 0, 0, 6, 0], [0, 0, 0, 0, 0], [1]),
    "late parent between the copies of a duplicate": ([1, 2, 5, 2, 6], [0, 0, 6, 0, 0], [0, 0, 0, 0, 0], [1]),
    "duplicate whose first copy is a parent": ([1, 2, 3, 2], [0, 0, 2, 0], [0, 0, 1, 0], [3]),
    "parent is a duplicate listed after its child": ([1, 4, 2, 2], [0, 2, 0, 0], [0, 0, 0, 0], [1]),
    "unknown proband": ([1, 2, 3], [0, 0, 1], [0, 0, 2], [3, 99, 98]),
    "unknown proband and a duplicate": ([1, 2, 2, 3], [0, 0, 0, 1], [0, 0, 0, 2], [99]),
    "unknown proband and a late father": ([1, 2, 3], [0, 3, 0], [0, 0, 0], [99]),
}
ENTRIES = ("genphi_simu_create", "genphi_ident_create", "genphi_implex_create")


def _spread(ids):
    """The same IDs far apart, the even ones negative: Ranks takes its hash map."""
    return [0 if i == 0 else (i * 1000003 if i % 2 else -i * 1000003) for i in ids]


def run_cases(capi):
    """{case: {entry point: [return code, genphi_last_error() or "" after a success]}} from the library capi (genlib_jl_amd._capi) loaded."""
    L = capi.lib()
    i64p = C.POINTER(C.c_int64)
    out = {}
    for name, case in CASES.items():
        for ids, lists in (("direct table", case), ("hash map", tuple(_spread(x) for x in case))):
            ind, fa, mo, pro = (np.asarray(x, dtype=np.int64) for x in lists)
            p = [a.ctypes.data_as(i64p) for a in (ind, fa, mo, pro)]
            anc, states = ind[:1].copy(), np.ones(1, dtype=np.int32)           # gen.simu: the first individual, state 1
            calls = {
                "genphi_simu_create": lambda h: L.genphi_simu_create(len(ind), p[0], p[1], p[2], len(pro), p[3], 1, anc.ctypes.data_as(i64p),
                                                                    states.ctypes.data_as(C.POINTER(C.c_int32)), 130, 7, 0, C.byref(h)),
                "genphi_ident_create": lambda h: L.genphi_ident_create(len(ind), p[0], p[1], p[2], len(pro), p[3], 130, 7, 0, 0, C.byref(h)),
                "genphi_implex_create": lambda h: L.genphi_implex_create(len(ind), p[0], p[1], p[2], len(pro), p[3], 0, C.byref(h)),
            }
            got = {}
            for entry in ENTRIES:
                h = C.c_void_p()
                rc = calls[entry](h)
                got[entry] = [int(rc), capi.last_error() if rc else ""]
                assert bool(h.value) == (rc == 0), (name, ids, entry)
                if h.value:
                    getattr(L, entry.replace("_create", "_destroy"))(h)
            out[name + ", " + ids] = got
    return out


def record(root, commit):
    sys.path.insert(0, root)
    from genlib_jl_amd import _capi
    assert os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__))) == os.path.abspath(root)
    return {"recorded_at_commit": commit, "cases": run_cases(_capi)}


def test_error_codes_and_texts_are_those_of_the_recorded_commit(gen):
    with open(GOLDEN) as f:
        want = json.load(f)["cases"]
    got = run_cases(gen._capi)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    # the cases do reach every code and both sides of every precedence
    codes = {tuple(v[e][0] for e in ENTRIES) for v in want.values()}
    C_ = gen._capi
    assert {(c, c, c) for c in (C_.GENPHI_OK, C_.GENPHI_ERR_UNKNOWN_ID, C_.GENPHI_ERR_DUPLICATE_ID, C_.GENPHI_ERR_ORDER)} == codes
    texts = " ".join(v[e][1] for v in want.values() for e in ENTRIES)
    for part in ("duplicate individual ID 2", ": father ", ": mother ", "KeyError: proband 99 not found", "KeyError: proband 99000297 not found",
                 "individual -2000006: father -4000012 is unknown"):
        assert part in texts, part
    assert want["late parent between the copies of a duplicate, direct table"] != want["late parent between the copies of a duplicate, hash map"]


if __name__ == "__main__":
    json.dump(record(sys.argv[1], sys.argv[2]), sys.stdout, indent=1)
    print()
