"""gen.sparse_phi at the wave widths where its kernels switch form, bit for bit against the slot oracle (oracle/slot_oracle.cpp,
itself equal to the literal dictionary restatement on every smaller case: tests/test_sparse_slot_oracle.py).

csrc/sparse_phi.hip picks a wave's kernels by its old set n_old: the fused row kernel with T in up to 48 KB of LDS, the same kernel
with 48-144 KB of dynamic LDS (kFusedMaxOld = 36,864 floats), and above that the two-kernel form whose new x new entries gather T from
HBM.  The proband block goes to the host through a pinned buffer up to 8,192 probands and through a plain 2D copy beyond; sweeps of
more than 4,096 waves record no per-wave events.  Every case first asserts from the host-only schedule that it reaches its path
(tests/wide_waves.py: check_regime); then every proband pair through K.get, info(), the `show` line, phiMean and the stored entries
are compared with the oracle."""
import numpy as np
import pytest

import wide_waves as W

pytestmark = pytest.mark.gpu


def _lexsorted(r, c, v):
    o = np.lexsort((v, c, r))
    return r[o], c[o], v[o]


def _compare(gen, K, want):
    ids = want.ids
    n = len(ids)
    step = max(1, (1 << 22) // max(n, 1))
    for a0 in range(0, n, step):                                  # every proband pair, a band of rows at a time
        a = np.repeat(ids[a0:a0 + step], n)
        b = np.tile(ids, min(step, n - a0))
        got, ref = K.get(a, b).astype(np.float32), want.get(a, b)
        bad = np.flatnonzero(got != ref)
        assert len(bad) == 0, (len(bad), [(int(a[k]), int(b[k]), float(got[k]), float(ref[k])) for k in bad[:5]])
    nr, nz, sa, sd = K.info()
    wr, wz, wa, wd = want.info()
    assert (nr, nz) == (wr, wz), ((nr, nz), (wr, wz))
    assert abs(sa - wa) <= 1e-12 * max(1.0, abs(wa)) and abs(sd - wd) <= 1e-12 * max(1.0, abs(wd)), ((sa, sd), (wa, wd))
    assert repr(K) == want.show()
    if nr > 1:
        assert gen.phiMean(K) == want.phi_mean()
    for x, y in zip(_lexsorted(*K.entries()), _lexsorted(*want.entries())):
        assert np.array_equal(x, y)


def _run(gen, oracle, name):
    ind, fa, mo, sex, pro, sort = W.case(name)
    n_old, n_new = W.check_regime(gen, name, ind, fa, mo, sex, pro, sort)
    K = gen.sparse_phi(gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=sort), pro)
    assert K.stats()["n_waves"] == len(n_new)
    want = oracle.SlotSparsePhi(oracle.Pedigree(ind, fa, mo, sort=sort), pro)
    try:
        _compare(gen, K, want)
        off = want.matrix()[~np.eye(len(want.ids), dtype=bool)]
        assert (off > 0).mean() > 0.005                               # not a funnel of unrelated couples
    finally:
        want.close()                                                  # (the oracle's live matrix: up to 6 GB of host memory)
    return K, n_old, n_new


def test_sparse_phi_fused_waves_at_their_lds_edges(gen, oracle):
    """Fused waves at n_old = 12,288 (48 KB of LDS), 12,289 (the first after hipFuncSetAttribute), 20,002 and 24,003 (T rows of
    2 and 3 mod 4 floats: padded quads), 36,864 (144 KB): survivors compacted by the trailing workgroups in every one."""
    _run(gen, oracle, "fused_lds_edges")


@pytest.mark.parametrize("name", ["two_kernel_skip", "two_kernel_one_parent"])
def test_sparse_phi_first_two_kernel_waves(gen, oracle, name):
    """n_old = 36,865 (the first wave of the automatic two-kernel form: every new row gathers T from HBM) and 38,2xx with 21,000 new
    rows, in a sweep whose other waves are fused; dragged survivors (parents two generations up) or one-parent members."""
    _run(gen, oracle, name)


def test_sparse_phi_two_kernel_waves_unsorted(gen, oracle, capfd, monkeypatch):
    """genealogy(...; sort=false) at width: entries that outlive their columns, some of them appended by the two-kernel waves.  Once
    with the default list, once with the list forced to overflow: the second sweep at full size."""
    name = "two_kernel_unsorted"
    ind, fa, mo, sex, pro, sort = W.case(name)
    n_old, n_new = W.check_regime(gen, name, ind, fa, mo, sex, pro, sort)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=False)
    want = oracle.SlotSparsePhi(oracle.Pedigree(ind, fa, mo, sort=False), pro)
    try:
        r, c, _ = want.entries()
        stale = ~np.isin(c, r[r == c])                                # entries whose column is not a proband: they outlived it
        n_stale = int(stale.sum())
        from genlib_jl_amd import _capi
        order, _, wave = _capi.sparse_schedule(ped.ind, ped.father, ped.mother, pro)
        wave_of = dict(zip(order.tolist(), wave.tolist()))
        two = set(np.flatnonzero((n_old > W.FUSED_MAX_OLD) & (n_new > 0)).tolist())
        # (rank = file position: every individual is an ancestor of a proband, none is pruned) some outliving entries of a proband
        # and a later member of the same two-kernel wave: appended by sparse_newnew_kernel, which gathers T from HBM there
        wr, wc = np.array([wave_of[int(ind[k - 1])] for k in r[stale]]), np.array([wave_of[int(ind[k - 1])] for k in c[stale]])
        assert ((wr == wc) & np.isin(wc, list(two))).sum() > 0 and np.isin(wc, list(two)).sum() > 0, n_stale
        monkeypatch.setenv("GENPHI_TRACE", "1")
        capfd.readouterr()
        K = gen.sparse_phi(ped, pro)
        assert capfd.readouterr().err.count("sweep done") == (1 if n_stale <= 65536 else 2)
        _compare(gen, K, want)
        monkeypatch.setenv("GENPHI_SPARSE_STALE_CAP", "1")
        K1 = gen.sparse_phi(ped, pro)
        assert capfd.readouterr().err.count("sweep done") == 2             # the list overflowed, the sweep ran twice
        _compare(gen, K1, want)
    finally:
        want.close()


def test_sparse_phi_result_copy_paths(gen, oracle):
    """The proband block through the pinned staging buffer (grown to 8,192 probands = 256 MB), through the plain 2D copy (8,193),
    then through the kept pinned buffer again."""
    for name in ("copy_small", "copy_8192", "copy_8193", "copy_small"):
        K, _, _ = _run(gen, oracle, name)
        assert K.info()[0] == {"copy_small": 103, "copy_8192": 8192, "copy_8193": 8193}[name]


def test_sparse_phi_more_than_4096_waves(gen, oracle):
    """4,201 waves: the sweep records no per-wave events and the band events of the result copy move to the front; then an ordinary
    call in the same process."""
    K, _, n_new = _run(gen, oracle, "many_waves")
    assert len(n_new) > 4096 and K.stats()["sweep_ms"] == 0.0            # (no events: no sweep time either)
    K, _, _ = _run(gen, oracle, "copy_small")
    assert K.stats()["sweep_ms"] > 0


def test_sparse_phi_bench_workloads(gen, oracle):
    """bench.py's two sparse workloads, compared instead of only timed: genea140 with all 140 probands (sparse140) and the
    1e5-individual / 2,000-proband / 20-generation synthetic pedigree (sparse2k)."""
    from genlib_jl_amd import synth
    g = oracle.read_tsv(gen.genea140)
    ped = gen.genealogy(gen.genea140)
    pro = gen.pro(ped)
    assert len(pro) == 140
    want = oracle.SlotSparsePhi(oracle.Pedigree(*g[:3]), pro)
    _compare(gen, gen.sparse_phi(ped, pro), want)
    want.close()
    ind, fa, mo, sex, pro = synth.random_mating(100_000, 2_000, 20)
    want = oracle.SlotSparsePhi(oracle.Pedigree(ind, fa, mo), pro)
    _compare(gen, gen.sparse_phi(gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}), pro), want)
    want.close()
