"""A refactor's speed check: the parent commit's build and this tree's, alternately, on one machine.
    parent_vs_new.py run PARENT_TREE FIRST LAST OUT     rounds FIRST..LAST (parent first in rounds 1-3, the new build first afterwards); per build
                                                        and round bench.py --full on cfg4 and call_wall.py on cfg2 (genea140) and cfg3; raw lines to OUT
    parent_vs_new.py run PARENT_TREE FIRST LAST OUT sweeps    the same for the sweep handles: per build and round profiles/simu_bench.py, ident_bench.py,
                                                        gc_bench.py and implex_bench.py at their defaults (parent first in the first half of FIRST..LAST)
    parent_vs_new.py summary OUT [OUT ...]              per figure min..max over the rounds, the median, and where the new median lies (of the sweep
                                                        scripts' lines: every time they print, the keys *_ms and call_ms_*)
PARENT_TREE is a checkout of the parent commit with its library built.  A command that fails ends the run: nothing more is started."""
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CMDS = [(300, ["python", "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-others", "--no-d2h"]),
        (120, ["python", "profiles/microbench/call_wall.py", "cfg2", "cfg3"])]
SWEEP_CMDS = [(240, ["python", "profiles/%s_bench.py" % s]) for s in ("simu", "ident", "gc", "implex")]


def run(parent, first, last, out_path, sweeps=False):
    trees = {"parent": os.path.abspath(parent), "new": ROOT}
    parent_first_until = (first + last) // 2 if sweeps else 3
    with open(out_path, "w") as out:
        for r in range(first, last + 1):
            for which in (("parent", "new") if r <= parent_first_until else ("new", "parent")):
                out.write(f"== {which} library, round {r}\n")
                for limit, cmd in (SWEEP_CMDS if sweeps else CMDS):
                    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=trees[which], capture_output=True, text=True)
                    out.write("".join(l + "\n" for l in p.stdout.splitlines() if l.startswith("{") or l.startswith("cfg")))
                    out.flush()
                    if p.returncode != 0:
                        out.write(f"!! exit status {p.returncode}: {' '.join(cmd)}\n{p.stderr[-3000:]}\n")
                        return 1
                print(f"{which} library, round {r}: done", flush=True)
    return 0


def summary(paths):
    fig, rounds, which = {}, set(), None

    def add(k, v):
        fig.setdefault(k, {"parent": [], "new": []})[which].append(float(v))
    for path in paths:
        for line in open(path):
            m = re.match(r"== (\w+) library, round (\d+)", line)
            if m:
                which = m.group(1)
                rounds.add(int(m.group(2)))
            elif line.startswith("{") and "end_to_end" not in line:
                j = json.loads(line)                                   # a line of a sweep's bench script (gc_bench.py's has no "what")
                for k, v in j.items():
                    if k.endswith("_ms") or k.startswith("call_ms_"):
                        add(f"{j.get('what', 'gc')} {j['workload']} {k}", v)
            elif line.startswith("{"):
                j = json.loads(line)
                e = j["end_to_end"]
                add("cfg4 bench ms_per_step", j["ms_per_step"])
                add("cfg4 bench plan_ms", e["plan_ms"])
                add("cfg4 bench first_call_ms", e["first_call_ms"])
                add("cfg4 one-shot call wall first_ms", e["call_wall"]["first_ms"])
            else:
                m = re.match(r"(cfg\d): gen.phi call wall median ([\d.]+) ms \(min ([\d.]+), max [\d.]+\); plan [\d.]+, first compute ([\d.]+), second compute ([\d.]+)", line)
                if m:
                    w = "genea140" if m.group(1) == "cfg2" else m.group(1)
                    for name, v in zip(("one-shot call wall median", "one-shot call wall min", "first compute", "second compute"), m.groups()[1:]):
                        add(f"{w} {name}", v)
    print(f"parent and new library alternately, rounds {sorted(rounds)}; per figure min..max over the rounds and the median (ms)")
    width = max(38, max(len(k) for k in fig))
    for k, d in fig.items():
        p, n = d["parent"], d["new"]
        mp, mn = statistics.median(p), statistics.median(n)
        if mn < min(p):
            verdict = "below the parent's spread"
        elif mn > max(p):
            verdict = "ABOVE the parent's spread"
        elif len(p) > 1 and min(n) >= max(p):
            verdict = "within the parent's spread, but ALL of the new range lies at or above the parent's maximum"
        elif len(p) > 1 and min(n) > mp and mn > sorted(p)[-2]:
            verdict = "within the parent's spread only through the parent's largest round"
        else:
            verdict = "within the parent's spread"
        print(f"{k:{width}s} parent {min(p):9.3f}..{max(p):9.3f} med {mp:9.3f} | new {min(n):9.3f}..{max(n):9.3f} med {mn:9.3f} ({mn / mp - 1:+.1%}) | new median {verdict}")


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"] and (len(sys.argv) == 6 or sys.argv[6:] == ["sweeps"]):
        sys.exit(run(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sweeps=len(sys.argv) == 7))
    assert sys.argv[1:2] == ["summary"] and len(sys.argv) > 2, __doc__
    summary(sys.argv[2:])
