"""Regenerate tests/golden/wh_derivs.json: the exact-derivative tier's truth (tests/wh_ref.py).

Nothing is read but tests/wh_ref.py's case table.  Per case and walker the file holds the inputs,
the 60-digit finite-difference truth of the per-epoch model RV and its first and second derivatives
(decimal strings of 30 digits), the two branch counters per level, and the float hyper-dual run.

    python tests/golden/make_wh_derivs.py [-j PROCESSES] [CASE ...]

About 3000 mpmath integrations (an hour of one CPU); they are spread over PROCESSES (default: the
CPUs of this machine).  Cases named on the command line replace those of an existing file.
"""
import argparse
import json
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import wh_ref as R  # noqa: E402


def _point(job):
    name, w, key, shifts = job
    st, rv, cnt = R.eval_point(R.case_inputs()[name], w, shifts)
    assert st == R.OK, (name, w, key, st)
    return name, w, key, rv, cnt  # (mpf pickles exactly)


def _record(job):
    name, w, runs, cnt = job
    R.mp.dps = R.TRUTH_DPS
    return name, w, R.make_walker_record(R.case_inputs()[name], w, runs, cnt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=os.cpu_count())
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    cases = R.case_inputs()
    names = a.cases or list(cases)
    jobs = [(n, w, key, sh) for n in names for w in range(len(cases[n]["walkers"])) for key, sh in R.fd_points(cases[n])]
    jobs.sort(key=lambda j: -len(cases[j[0]]["levels"]) * len(cases[j[0]]["walkers"][0]))  # long runs first
    runs, cnts = {}, {}
    with multiprocessing.Pool(a.j) as pool:
        for k, (n, w, key, rv, cnt) in enumerate(pool.imap_unordered(_point, jobs, chunksize=4)):
            runs.setdefault((n, w), {})[key] = rv
            if key == "0":
                cnts[(n, w)] = cnt
            if k % 200 == 0:
                print(f"{k}/{len(jobs)} integrations", flush=True)
        recs = pool.map(_record, [(n, w, r, cnts[(n, w)]) for (n, w), r in runs.items()], chunksize=1)
    out = R.load_fixture() if a.cases and os.path.exists(R.FIXTURE) else {}
    for n in names:
        out[n] = dict(cases[n], walkers_out=[None] * len(cases[n]["walkers"]))
    for n, w, rec in recs:
        out[n]["walkers_out"][w] = rec
    out = {n: out[n] for n in cases if n in out}
    with open(R.FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(c, separators=(',', ':'))}" for n, c in out.items()) + "\n}\n")
    print(f"wrote {R.FIXTURE}: {os.path.getsize(R.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
