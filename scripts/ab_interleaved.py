#!/usr/bin/env python3
"""Interleaved A/B of `bench.py --gpus 1` between copies of the package (each
run a fresh child process of scripts/ab_run.py), e.g. a parent build kept
under ab_old/ against the tree:
    ab_interleaved.py OUT.json ROUNDS parent=ab_old new=. -- --steps 30 --warmup 10
    (name=pkgroot[:module.ATTR=val,...]; "." = this tree)
Prints every run's ms/step and last loss, then per arm the median, range and
the set of last losses. Stops at the first failing run."""
import json
import os
import statistics
import subprocess
import sys

out, rounds = sys.argv[1], int(sys.argv[2])
i = sys.argv.index("--")
arms = []
for a in sys.argv[3:i]:
    name, spec = a.split("=", 1)
    root, _, ov = spec.partition(":")
    arms.append((name, root, [o for o in ov.split(",") if o]))
bargs = sys.argv[i + 1:]
res = {n: [] for n, _, _ in arms}
loss = {n: set() for n, _, _ in arms}
for r in range(rounds):
    for name, root, ov in arms:
        env = dict(os.environ)
        if root != ".":
            env["TDG_PKG_ROOT"] = root
        cmd = ["timeout", "-k", "10", "150", sys.executable, "scripts/ab_run.py"] + ov + ["--", "--gpus", "1"] + bargs
        p = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if p.returncode != 0:
            print(name, "FAILED rc", p.returncode, p.stderr[-2000:], flush=True)
            sys.exit(1)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        j = json.loads(line)
        res[name].append(j["ms_per_step"])
        loss[name].add(j["config"].get("last_loss"))
        print(r, name, j["ms_per_step"], j["config"].get("last_loss"), flush=True)
summ = {}
for n in res:
    v = res[n]
    summ[n] = {"runs": v, "median": statistics.median(v), "min": min(v), "max": max(v),
               "range": round(max(v) - min(v), 4), "last_loss": sorted(loss[n])}
print(json.dumps(summ), flush=True)
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump({"args": bargs, "arms": summ}, open(out, "w"), indent=1)
