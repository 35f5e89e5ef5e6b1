"""Random differential stress of the five queries that read the resident Float32 result in place (not part of the pytest run by itself;
tests/test_queries_random.py runs a short fixed-seed round of it):
    python tests/stress_queries.py [n_cases] [seed]
The pedigrees, proband lists and sweep knobs are those of tests/stress_random.py (FULL / SPLIT / WIDE last steps, certified and exact
rows, the plain and the persistent proband-order pass, a proband cut delivered from the slot matrix, the sparse leading cuts, the fused
small-level run, row shards ...), capped at 400 probands and 7,000 individuals.  On top of them, from a generator of its own:
a device cache soiled with positive floats before the plan is created, a sequence of 3 - 6 resident states on ONE plan (full results,
unaligned / one-row / last-row / empty shards, kernel = 1, no_sparse, a smaller after a larger result and the reverse, a Float64 result
in between, release_device), and after every compute_device the host copy against the compiled oracle bit for bit, then
genphi_result_sums, genphi_result_group_sums, genphi_result_over, genphi_result_nearest and genphi_result_bootstrap against the Python
oracles of tests/*_oracle.py applied to that host copy.

What the queries rely on and no interface states: the padding columns [N, ld) of every resident row are +0 after every
delivery path, ld % 64 == 0, and res_ld / res_row_begin / res_n_rows and the phiOver offset cache (genphi_plan::over, dropped by
set_resident_rows) follow every compute.  A stale positive float in the
padding shows in the sums and the bootstrap, a wrong row_begin in every list.

No tolerance but the two derived rules that are in the tree with their derivation: group_sums_oracle.gamma for the Float64 sums and the
bound of tests/test_phi_ci_gpu.py for the bootstrap (`==` where phi_ci_oracle.exact_precondition holds).  No case is skipped; a generator
that leaves a stated range is a failure of the case.  Prints one `FAIL case=...` line per failing case with everything needed to replay it
(tests/query_case.py <case>), and a summary."""
import ctypes
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
os.environ["GENPHI_ENV_HOOKS"] = "1"      # (stress_random sets it too; the knobs of a case reach its plan through tuning=, not the environment)

import group_sums_oracle as GO          # noqa: E402
import phi_ci_oracle as CO              # noqa: E402
import phi_nearest_oracle as NO         # noqa: E402
import phi_over_oracle as OO            # noqa: E402
import stress_random as SR              # noqa: E402

MAX_PRO, MAX_IND = 400, 7000
U = 2.0 ** -53
B_CHOICES, B_WEIGHTS = [1, 65, 130], [0.45, 0.4, 0.15]          # (the oracle of 130 resamples of 400 probands adds up 2e7 terms by math.fsum)
KINDS = ["full", "shard", "one_row", "last_row", "empty", "kernel1", "no_sparse", "full_after_smaller", "shard_after_larger", "f64_then_f32",
         "release_then_compute"]
PAIRS = {"full_after_smaller", "shard_after_larger", "f64_then_f32"}       # kinds of two resident states
PLAN_KNOBS = [k for k in SR.KNOBS if k != "GENPHI_SPARSE_NO_FUSED"]        # (that one steers gen.sparse_phi, which has no plan)


def _distinct(pro):
    return list(dict.fromkeys(int(x) for x in pro))


def _base_case(case):
    """stress_random's draws of `case`, or of the first deterministic redraw of it that fits the cap."""
    for attempt in range(64):
        c = case if attempt == 0 else int(np.random.default_rng([case, 6, attempt]).integers(1 << 30))
        r, n_gen, n_ind, n_pro, skip, ind, fa, mo, sex, pro, env = SR.make_case(c)
        sort = bool(r.random() < 0.5)                                      # the coin of stress_random.run_case
        if len(ind) <= MAX_IND and len(_distinct(pro)) <= MAX_PRO:
            return c, ind, fa, mo, sex, pro, env, sort
    raise AssertionError("64 redraws of case %d all exceed the cap" % case)


def _unaligned_shard(q, n):
    """(a, b), 0 < a < b <= n, neither a multiple of 4 (so none of 64)."""
    a_ok = [x for x in range(1, n) if x % 4]
    a = int(q.choice(a_ok))
    b_ok = [x for x in range(a + 1, n + 1) if x % 4]
    if not b_ok:                                                           # (a = n - 1 and n a multiple of 4)
        a = int(q.choice([x for x in a_ok if any(y % 4 for y in range(x + 1, n + 1))]))
        b_ok = [x for x in range(a + 1, n + 1) if x % 4]
    return a, int(q.choice(b_ok))


def _draw_states(q, n):
    """3 - 6 resident states: dicts(kind, rows = None | (a, b), kernel, no_sparse, f64, release)."""
    want = int(q.integers(3, 7))

    def st(kind, rows=None, **kw):
        d = dict(kind=kind, rows=rows, kernel=0, no_sparse=False, f64=False, release=False)
        d.update(kw)
        return d

    def any_rows(empty_ok=False):
        u = q.random()
        if empty_ok and u < 0.15:
            a = int(q.integers(1, n + 1))
            return a, a
        return None if u < 0.5 else _unaligned_shard(q, n)

    states = []
    while len(states) < want:
        kinds = [k for k in KINDS if len(states) + (2 if k in PAIRS else 1) <= want]
        kind = str(q.choice(kinds))
        if kind == "full":
            states.append(st(kind))
        elif kind == "shard":
            states.append(st(kind, _unaligned_shard(q, n)))
        elif kind == "one_row":
            a = int(q.integers(0, n))
            states.append(st(kind, (a, a + 1)))
        elif kind == "last_row":
            states.append(st(kind, (n - 1, n)))
        elif kind == "empty":
            a = int(q.integers(1, n + 1))                                  # ((0, 0) asks for every row)
            states.append(st(kind, (a, a)))
        elif kind == "kernel1":
            states.append(st(kind, any_rows(), kernel=1))
        elif kind == "no_sparse":
            states.append(st(kind, any_rows(), no_sparse=True))
        elif kind == "full_after_smaller":
            states += [st("smaller", _unaligned_shard(q, n)), st(kind)]
        elif kind == "shard_after_larger":
            states += [st("larger"), st(kind, _unaligned_shard(q, n))]
        elif kind == "f64_then_f32":
            states += [st("f64", any_rows(), f64=True), st("f32_after_f64", any_rows(empty_ok=True))]
        else:
            states.append(st(kind, any_rows(), release=True))
    for s in states:                                                       # what every query of the state is asked
        kmax = min(n - 1, 64)
        s["k"] = int(q.choice([1, min(2, kmax), kmax, int(q.integers(1, kmax + 1))]))
        s["G"] = int(q.choice([1, 2, 7, 64, n]))
        s["label_seed"] = int(q.integers(1 << 30))
        s["b"] = int(q.choice(B_CHOICES, p=B_WEIGHTS))
        s["entry"] = (float(q.random()), float(q.random()))               # the entry of the resident rows that becomes a threshold
    return states


def make_case(case):
    """Everything of one random case, a pure function of `case`: dict(case, base, ind, father, mother, sex, sort, pro, n, variant, env, tuning,
    soil, states, stale, seed)."""
    base, ind, fa, mo, sex, pro, env, sort = _base_case(case)
    q = np.random.default_rng([case, 6])
    pro = np.asarray(pro, dtype=np.int64)
    # the proband list of stress_random (duplicates, ancestors, every individual), or a part of it that the sizes of a random list never hit
    u, variant = q.random(), "as drawn"
    d = _distinct(pro)
    if u < 0.07:
        variant, pro = "two", np.array([d[0], d[1], d[0]], dtype=np.int64)
    elif u < 0.14:
        founders = ind[(fa == 0) & (mo == 0)]
        f = q.choice(founders, size=min(int(q.integers(2, 13)), len(founders)), replace=False)
        variant, pro = "founders", np.concatenate([f, f[:1]]).astype(np.int64)
    elif u < 0.22 and len(d) >= 64:
        keep = set(d[: 64 * int(q.integers(1, len(d) // 64 + 1))])
        variant, pro = "x64", np.array([x for x in pro if int(x) in keep], dtype=np.int64)          # (the repeats of the kept ones stay)
    elif u < 0.52:
        # probands at every depth, as stress_random's "share of all individuals" (which the cap on N redraws almost always): nobody
        # leaves the cuts, and about one such plan in six keeps the proband cut in place and delivers from the slot matrix
        share = q.permutation(ind)[: min(MAX_PRO, max(3, len(ind) // int(q.integers(1, 6))))]
        variant, pro = "every depth", np.concatenate([share, share[:2]]).astype(np.int64)
    n = len(_distinct(pro))
    assert 2 <= n <= MAX_PRO, "the generator left the range of the queries: %d probands" % n
    tuning = {k: v for k, v in env.items() if k in PLAN_KNOBS}
    if q.random() < 0.5:
        tuning["NEAREST_BUF"] = "128"
    panel = [1, 7, 64, None][int(q.integers(0, 4))]
    if panel is not None:
        tuning["BOOT_PANEL"] = str(panel)
    soil = bool(q.random() < 0.5)
    states = _draw_states(q, n)
    ok = [i for i in range(len(states) - 1) if not states[i]["f64"]]       # count there, recompute, then fill with the old count as cap
    stale = ok[int(q.integers(0, len(ok)))]
    return dict(case=case, base=base, ind=ind, father=fa, mother=mo, sex=sex, sort=sort, pro=pro, n=n, variant=variant, env=env, tuning=tuning,
                soil=soil, states=states, stale=stale, seed=int(q.integers(1 << 62)))


def rows_of(s, n):
    return (0, n) if s["rows"] is None else s["rows"]


def show_state(s):
    out = s["kind"] + ("" if s["rows"] is None else "(%d,%d)" % s["rows"])
    return out + (" kernel=1" if s["kernel"] else "") + (" no_sparse" if s["no_sparse"] else "") + (" f64" if s["f64"] else "") + \
        (" released" if s["release"] else "")


def describe(c):
    return "base=%d n_ind=%d n_pro=%d (%s) sort=%s soil=%s env=%s states=[%s]" % (
        c["base"], len(c["ind"]), c["n"], c["variant"], c["sort"], c["soil"], c["tuning"], ", ".join(show_state(s) for s in c["states"]))


def soiling_pedigree(n_pro):
    """Everybody but the founding couple descends from it, so every kinship among the probands (the last generation) is > 0."""
    r = np.random.default_rng(n_pro)
    sizes = [8, max(n_pro, 8), n_pro]
    ind, fa, mo = [1, 2], [0, 0], [0, 0]
    prev = [(1, 2)]                                                        # couples of the generation above
    for g, m in enumerate(sizes):
        first = len(ind) + 1
        for k in range(m):
            f, mth = prev[int(r.integers(len(prev)))]
            ind.append(first + k); fa.append(f); mo.append(mth)
        ids = np.arange(first, first + m)
        prev = [(int(a), int(b)) for a, b in zip(r.permutation(ids), r.permutation(ids)) if a != b] or [(first, first + 1)]
    return np.array(ind), np.array(fa), np.array(mo), np.arange(len(ind) - sizes[-1] + 1, len(ind) + 1)


def soil(gen, n_pro):
    """A plan whose level matrices and result hold only positive floats, computed and closed: its blocks wait in the device cache."""
    ind, fa, mo, pro = soiling_pedigree(max(n_pro, 2))
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)
    pl = gen.plan(ped, pro, tuning={})
    try:
        phi = pl.compute()
    finally:
        pl.close()
    return bool(phi.shape == (len(pro), len(pro)) and np.all(phi > 0))


def labels_of(s, n):
    """(form-0 labels, random labels) of a state, int32 with some -1: whole runs in shuffled group order, and any labelling."""
    r = np.random.default_rng(s["label_seed"])
    G = s["G"]
    n_runs = int(r.integers(1, min(G + 2, n) + 1))
    cuts = np.sort(r.choice(np.arange(1, n), size=n_runs - 1, replace=False)) if n_runs > 1 else np.zeros(0, dtype=np.int64)
    names = list(r.permutation(G)[:n_runs]) + [-1] * max(n_runs - G, 0)    # (more runs than groups: the others are runs of -1)
    names = r.permutation(np.array(names[:n_runs]))
    runs = np.zeros(n, dtype=np.int32)
    for k, (a, b) in enumerate(zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [n]]))):
        runs[a:b] = names[k]
    anyhow = r.integers(-1, G, size=n).astype(np.int32)
    return runs, anyhow


def form_of(labels):
    """0 when the probands of every group are one run of the proband order."""
    for g in np.unique(labels[labels >= 0]):
        at = np.nonzero(labels == g)[0]
        if at[-1] - at[0] + 1 != len(at):
            return 1
    return 0


def boot_within_bound(got, ref, n_rows, n):
    """tests/test_phi_ci_gpu.py::_within_bound (include/genphi.h: quad within 3 n_rows N 2^-53 relative, self within n_rows 2^-53)."""
    return bool(np.all(np.abs(got[0] - ref[0]) <= 3 * n_rows * n * U * ref[0]) and np.all(np.abs(got[1] - ref[1]) <= n_rows * U * ref[1]))


class Clock:
    """CPU seconds spent in the oracles."""
    total = 0.0

    def __enter__(self):
        self.t = time.process_time()

    def __exit__(self, *exc):
        Clock.total += time.process_time() - self.t


def check_queries(gen, pl, c, s, host, what, say, counts_of):
    """Every query of one Float32 state against the oracles on its host copy."""
    n, seed = c["n"], c["seed"]
    r0, r1 = rows_of(s, n)
    nr = r1 - r0

    def note(name, ok, detail=""):
        say("  %-34s %s" % (name, "ok" if ok else "DIFFERS " + detail))
        if not ok:
            what.append("%s: %s" % (show_state(s), name))

    # --- genphi_result_sums
    a, d, rows = pl.result_sums()
    with Clock():
        fd = math.fsum(float(host[k, r0 + k]) for k in range(nr))
        fa = math.fsum(host.astype(np.float64).ravel().tolist())
        bound = float(GO.gamma(nr * n)) * fa
    note("sums: rows", rows == nr, "%d, expected %d" % (rows, nr))
    note("sums: diagonal", d == fd, "%r, fsum %r" % (d, fd))
    note("sums: total", abs(a - fa) <= bound, "%r, fsum %r, bound %r" % (a, fa, bound))
    if nr == n:
        note("phi_mean", pl.phi_mean() == np.float32((a - d) / (n * n - n)))
    else:
        try:
            pl.phi_mean()
            note("phi_mean on a shard raises", False)
        except ValueError:
            note("phi_mean on a shard raises", True)
    # --- genphi_result_group_sums
    for name, lab in zip(("runs", "any"), labels_of(s, n)):
        got = pl.group_sums(lab, s["G"])
        with Clock():
            ref = GO.group_sums(host, lab, s["G"], row_begin=r0)
            try:
                GO.assert_within_rule(got[0], got[1], ref)
                bad = ""
            except AssertionError as e:
                bad = str(e)
        note("group_sums %s G=%d" % (name, s["G"]), bad == "", bad)
        note("group_sums %s: form, rows, cols" % name, got[4] == form_of(lab) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]),
             "form %d, expected %d" % (got[4], form_of(lab)))
        again = pl.group_sums(lab, s["G"])
        note("group_sums %s: same bits again" % name, all(x.tobytes() == y.tobytes() for x, y in zip(got[:4], again[:4])))
        if nr == 0:
            note("group_sums %s: zeros" % name, not got[0].any() and not got[1].any() and not got[2].any())
    # --- genphi_result_over
    if nr:
        e = host[int(s["entry"][0] * nr), int(s["entry"][1] * n)]
        thresholds = [-math.inf, 0.0, float(e), float(np.nextafter(np.float64(e), np.inf)), float(host.max()) * 2 + 1]
    else:
        thresholds = [-math.inf, 0.0, 0.25, 2.0]
    for t in thresholds:
        got = pl.phi_over(t)
        with Clock():
            ref = OO.over_numpy(host, t, r0)
        note("phi_over %r: %d pairs" % (t, len(ref[0])), OO.same(got, ref) and pl.count_over(t) == len(ref[0]), "%d pairs listed" % len(got[0]))
    # --- genphi_result_nearest
    k = s["k"]
    got = pl.nearest(k)
    with Clock():
        ref = NO.nearest_numpy(host, k, r0)
    note("nearest k=%d" % k, NO.same(got, ref))
    note("nearest: columns in [0, N), never the diagonal", got[0].shape == (nr, k) and (nr == 0 or (got[0].min() >= 0 and got[0].max() < n and
         not np.any(got[0] == (r0 + np.arange(nr))[:, None]))))
    # --- genphi_result_bootstrap
    b = s["b"]
    got = pl.bootstrap(b, seed)
    with Clock():
        full = np.zeros((n, n), dtype=np.float64)                          # (the oracle indexes the N x N matrix; it reads the given rows only)
        full[r0:r1] = host
        exact = CO.exact_precondition(full, counts_of(b))
        ref = CO.bootstrap(full, seed, 0, b, row_begin=r0, row_end=r1, exact=exact)
    if exact:
        note("bootstrap b=%d ==" % b, np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]))
    else:
        note("bootstrap b=%d within the bound" % b, boot_within_bound(got, ref, nr, n))
    note("bootstrap: finite", bool(np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))))
    if nr == 0:
        note("bootstrap: zeros", not got[0].any() and not got[1].any())


def check_refusals(gen, pl, c, s, what, say):
    """A Float64 result: every query refuses it (ValueError, as the test file of each says)."""
    n = c["n"]
    lab = np.zeros(n, dtype=np.int32)
    for name, call in (("result_sums", lambda: pl.result_sums()), ("group_sums", lambda: pl.group_sums(lab, 1)), ("count_over", lambda: pl.count_over(0.0)),
                       ("phi_over", lambda: pl.phi_over(0.0)), ("nearest", lambda: pl.nearest(1)), ("bootstrap", lambda: pl.bootstrap(1, c["seed"]))):
        try:
            call()
            ok = False
        except ValueError:
            ok = True
        say("  %-34s %s" % (name + " refuses a Float64 result", "ok" if ok else "ANSWERED"))
        if not ok:
            what.append("%s: %s answered a Float64 result" % (show_state(s), name))


def stale_fill(gen, pl, c, s, host, t, cap, what, say):
    """genphi_result_over's writing form on a NEW result with the count of the previous one as cap: it must count again."""
    n = c["n"]
    r0, r1 = rows_of(s, n)
    size = max(cap, 1)
    rows, cols, vals = np.full(size, -7, dtype=np.int32), np.full(size, -7, dtype=np.int32), np.full(size, -7, dtype=np.float32)
    got_n = ctypes.c_int64(-1)
    i32, f32 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    rc = gen._capi.lib().genphi_result_over(pl._h, ctypes.c_double(t), cap, rows.ctypes.data_as(i32), cols.ctypes.data_as(i32), vals.ctypes.data_as(f32),
                                            ctypes.byref(got_n))
    if s["f64"]:
        ok = rc == gen._capi.GENPHI_ERR_ARG and np.all(rows == -7)
    else:
        ref = OO.over_numpy(host, t, r0)
        m = len(ref[0])
        ok = rc == 0 and got_n.value == m
        if ok and m <= cap:
            ok = OO.same((rows[:m], cols[:m], vals[:m]), ref) and np.all(rows[m:] == -7)
        elif ok:
            ok = bool(np.all(rows == -7) and np.all(cols == -7))             # cap < count: nothing is written
    say("  %-34s %s" % ("over: old count %d as cap" % cap, "ok" if ok else "DIFFERS (rc %d, %d pairs)" % (rc, got_n.value)))
    if not ok:
        what.append("%s: phi_over filled from stale counts" % show_state(s))


def run_case(case, gen, O, report=None, make=make_case):
    """One case end to end.  Returns (list of the comparisons that failed, the case).  report: a function that gets one line per state and
    query (tests/query_case.py)."""
    c = make(case)
    say = report or (lambda line: None)
    what = []
    n = c["n"]
    pl = None
    try:
        ind, fa, mo, sex = c["ind"], c["father"], c["mother"], c["sex"]
        if not c["sort"]:
            from genlib_jl_amd import synth
            ind, fa, mo, sex = synth.parents_first_shuffle(ind, fa, mo, sex, seed=c["base"] & 0xffff)
        ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=c["sort"])
        with Clock():
            oped = O.Pedigree(ind, fa, mo, sort=c["sort"])
            want = oped.phi(c["pro"])
            want64 = oped.phi64(c["pro"]) if any(s["f64"] for s in c["states"]) else None
        assert want.shape == (n, n)
        if c["soil"] and not soil(gen, n):
            what.append("the soiling plan has an entry that is not positive")
        pl = gen.plan(ped, c["pro"], tuning=c["tuning"])
        modes = pl.step_modes()
        last = len(modes) - 1
        say("  plan: last step %s, proband cut in place: %s, %d level steps, cuts %s" % (
            "none" if last < 0 else ["FULL", "SPLIT", "WIDE"][modes[last]], bool(last >= 0 and pl.step_slots(last)[0] & 1), len(modes),
            pl.levels()[0][-3:]))
        counts = {}

        def counts_of(b):
            if b not in counts:
                counts[b] = CO.counts(n, c["seed"], 0, b)
            return counts[b]

        pending = None                                                     # (threshold, count) of the state before
        for i, s in enumerate(c["states"]):
            r0, r1 = rows_of(s, n)
            if s["release"]:
                pl.release_device()
            pl.compute_device(kernel=s["kernel"], rows=s["rows"], storage64=s["f64"], no_sparse=s["no_sparse"])
            say(" state %d: %s%s" % (i, show_state(s), "" if i else " (sparse cut %d)" % pl.sparse_levels()[0]))
            if s["f64"]:
                same = np.array_equal(pl.result_to_host_f64(), want64[r0:r1])
                host = None
            else:
                host = pl.result_to_host()
                same = host.shape == (r1 - r0, n) and np.array_equal(host.view(np.int32), want[r0:r1].view(np.int32))
                _, ld, rb, nrows = pl.result_device()
                ok = (rb, nrows) == (r0, r1 - r0) and ld % 64 == 0 and ld >= n
                say("  %-34s %s" % ("result_device", "ok" if ok else "ld %d, rows from %d, %d rows" % (ld, rb, nrows)))
                if not ok:
                    what.append("%s: result_device" % show_state(s))
            say("  %-34s %s" % ("host copy == oracle", "ok" if same else "DIFFERS"))
            if not same:
                what.append("%s: host copy" % show_state(s))
            if pending is not None:
                stale_fill(gen, pl, c, s, host, pending[0], pending[1], what, say)
                pending = None
            if s["f64"]:
                check_refusals(gen, pl, c, s, what, say)
                continue
            check_queries(gen, pl, c, s, host, what, say, counts_of)
            if i == c["stale"]:
                nr = r1 - r0
                t = float(host[int(s["entry"][1] * nr), int(s["entry"][0] * n)]) if nr else 0.0
                pending = (t, pl.count_over(t))                            # the last counting pass before the next compute
    except Exception as e:          # noqa: BLE001
        what.append("exception %s: %s" % (type(e).__name__, e))
        say("  " + what[-1])
    finally:
        if pl is not None:
            pl.close()
    return what, c


def main():
    import genlib_jl_amd as gen
    from oracle import oracle as O
    O.fit_threads_to_quota()
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 12345
    rng = np.random.default_rng(seed0)
    t0, n_fail, n_states = time.time(), 0, 0
    for k in range(n_cases):
        case = int(rng.integers(1 << 30))
        what, c = run_case(case, gen, O)
        n_states += len(c["states"])
        if what:
            n_fail += 1
            print("FAIL case=%d env=%s states=[%s] -> %s" % (case, c["tuning"], ", ".join(show_state(s) for s in c["states"]), what), flush=True)
        if (k + 1) % 20 == 0:
            print("... %d cases, %d failures, %.0f s" % (k + 1, n_fail, time.time() - t0), flush=True)
    print("query stress: %d cases, %d failures in %.1f s (%d resident states, %.1f s of CPU in the oracles, seed %d)" % (
        n_cases, n_fail, time.time() - t0, n_states, Clock.total, seed0), flush=True)
    return 1 if n_fail else 0


if __name__ == "__main__":
    sys.exit(main())
