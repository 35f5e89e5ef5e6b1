"""gen.gc (src/compute.jl:518-595) on the CPU: the two oracles of tests/gc_oracle.py against each other and against the
reference's pin, the reference's quirks on hand-built pedigrees, the divergence of the reference's Float32 path sums from
the correctly rounded value past 24 steps, and the host-only parts of the library's gen.gc (argument errors, exports)."""
import ctypes
import os
import re

import numpy as np
import pytest

from gc_oracle import ExactGC, divergence_pedigree, gc_exact_rows, gc_literal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ped(gen, ind, fa, mo, sort=True):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=sort)


def quirk_pedigree(gen):
    """1, 2, 5, 10, 11 founders; 3 = (1, 2); 4 = (1, -) one parent; 6 = (3, 5); 7 = (3, 4); 8 = (6, 7) and 9 = (4, -) leaves;
    10 and 11 founders without children."""
    ind = np.arange(1, 12)
    fa = np.array([0, 0, 1, 1, 0, 3, 3, 6, 4, 0, 0])
    mo = np.array([0, 0, 2, 0, 0, 5, 4, 7, 0, 0, 0])
    return _ped(gen, ind, fa, mo)


# pro: a leaf, a one-parent leaf, the first leaf again (quirk 2), a non-leaf (quirk 1), a founder leaf that is also an ancestor
# ancestors: 1 twice (quirk 3), 3 with parents (quirk 5), 8 a leaf proband (quirk 4), 10, 5, and 11 unrelated (quirk 6)
QUIRK_PRO = [8, 9, 8, 3, 10]
QUIRK_ANC = [1, 1, 3, 8, 10, 5, 11]
QUIRK_EXPECTED = np.array([
    [0.375, 0.375, 0.5, 1.0, 0.0, 0.25, 0.0],     # 8: 1 -> 3 -> 6 -> 8, 1 -> 3 -> 7 -> 8, 1 -> 4 -> 7 -> 8; 3 twice; itself
    [0.25, 0.25, 0.0, 0.0, 0.0, 0.0, 0.0],        # 9: 1 -> 4 -> 9
    [0.0] * 7,                                    # 8 again: its accumulator was reset after being read
    [0.0] * 7,                                    # 3 has children: never a leaf
    [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0],          # 10: its own column
], dtype=np.float32)


def test_literal_is_exact_on_bundled_pedigrees(gen):
    for path in (gen.geneaJi, gen.genea140):
        ped = gen.genealogy(path)
        pro, anc = gen.pro(ped), gen.founder(ped)
        lit = gc_literal(ped.ind, ped.father, ped.mother, pro, anc)
        exact = gc_exact_rows(ped.ind, ped.father, ped.mother, pro, anc)
        assert lit.shape == (len(pro), len(anc))
        assert np.array_equal(lit.view(np.int32), exact.view(np.int32))


def test_literal_genea140_pin(gen):
    ped = gen.genealogy(gen.genea140)
    lit = gc_literal(ped.ind, ped.father, ped.mother, gen.pro(ped), gen.founder(ped))
    assert lit.shape == (140, 7399)
    assert float(np.sum(lit, dtype=np.float64)) == 140.0          # test/runtests.jl:28: sum(gen.gc(ped)) == 140


def test_quirks_in_both_oracles(gen):
    ped = quirk_pedigree(gen)
    lit = gc_literal(ped.ind, ped.father, ped.mother, QUIRK_PRO, QUIRK_ANC)
    exact = gc_exact_rows(ped.ind, ped.father, ped.mother, QUIRK_PRO, QUIRK_ANC)
    assert np.array_equal(lit, QUIRK_EXPECTED)
    assert np.array_equal(exact, QUIRK_EXPECTED)


def test_quirk_unknown_and_empty_in_oracles(gen):
    ped = quirk_pedigree(gen)
    with pytest.raises(KeyError):
        gc_literal(ped.ind, ped.father, ped.mother, [8, 99], [1])
    with pytest.raises(KeyError):
        gc_literal(ped.ind, ped.father, ped.mother, [8], [99])
    assert gc_literal(ped.ind, ped.father, ped.mother, [], [1, 2]).shape == (0, 2)
    assert gc_literal(ped.ind, ped.father, ped.mother, [8, 9], []).shape == (2, 0)


def test_literal_diverges_from_exact_past_24_steps(gen):
    """The reference adds 128 paths of 2^-30 to 0.25 one at a time: each is below half an ulp and lost.  The exact
    contribution 0.25 + 2^-23 is a Float32; this is what gen.gc returns (test_gc_gpu.py), not the reference's 0.25."""
    ind, fa, mo, sex, P, A = divergence_pedigree()
    ped = _ped(gen, ind, fa, mo)
    lit = gc_literal(ped.ind, ped.father, ped.mother, [P], [A])
    ex = ExactGC(ped.ind, ped.father, ped.mother)
    w = ex.rows([P], [A], exact_ints=True)[0, 0]
    assert w * 2 ** 23 == (2 ** 21 + 1) * 2 ** ex.S            # 0.25 + 2^-23, exactly
    assert lit[0, 0] == np.float32(0.25)
    assert ex.rows([P], [A])[0, 0] == np.float32(0.25 + 2.0 ** -23)


def test_gc_unknown_ids_raise_without_gpu(gen):
    ped = quirk_pedigree(gen)
    with pytest.raises(KeyError):
        gen.gc(ped, pro=[8, 99])
    with pytest.raises(KeyError):
        gen.gc(ped, pro=[8], ancestors=[1, 99])
    with pytest.raises(KeyError):
        gen.GCPlan(ped.ind, ped.father, ped.mother, [8], [0])


def test_gc_plan_is_host_only(gen):
    """genphi_gc_create plans on the host: the handle exists (and reports its slot rows) before any GPU is touched."""
    ped = gen.genealogy(gen.genea140)
    h = gen.GCPlan(ped.ind, ped.father, ped.mother, gen.pro(ped), gen.founder(ped))
    try:
        st = h.stats()
        assert h.shape == (140, 7399)
        assert st["peak_slots"] > 0 and st["sweep_ms"] == 0.0
    finally:
        h.close()


def test_julia_shim_symbols_are_exported(gen):
    from genlib_jl_amd import _capi
    src = open(os.path.join(ROOT, "genlib.jl_amd", "julia", "GenLibAMD.jl")).read()
    called = set(re.findall(r"\(:(genphi_gc_[a-z_]+), libgenphi\)", src))
    assert called == {"genphi_gc_create", "genphi_gc_compute", "genphi_gc_result_to_host", "genphi_gc_destroy"}
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name in called | {"genphi_gc_result_device", "genphi_gc_stats"}:
        assert hasattr(L, name), name
