"""Regenerate tests/golden/stability_truth.json: the stability screen's truth (tests/stability_ref.py).

Nothing is read but tests/stability_ref.py's case table.  Per case the file holds the inputs and, per state, the
40-digit run's status, step count, final xv and ext (decimal strings of 30 digits) and its decision margins: the
d^2 / dmin2 and the |r| / r_max closest to 1 that the run met.

    python tests/golden/make_stability_truth.py [-j PROCESSES] [CASE ...]

About 12000 mpmath Kepler steps (a few minutes of one CPU), spread over PROCESSES (default 8).  Cases named on
the command line replace those of an existing file.
"""
import argparse
import json
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import stability_ref as R  # noqa: E402


def _state(job):
    name, i = job
    return name, i, R.record(R.run_case(R.cases()[name], R.mpf, states=[i])[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    cases = R.cases()
    names = a.cases or list(cases)
    jobs = [(n, i) for n in names for i in range(len(cases[n]["states"]))]
    jobs.sort(key=lambda j: -cases[j[0]]["n_blocks"] * cases[j[0]]["sample_every"] * len(cases[j[0]]["states"][0]))
    out = R.load_fixture() if a.cases and os.path.exists(R.FIXTURE) else {}
    for n in names:
        out[n] = dict(cases[n], truth=[None] * len(cases[n]["states"]))
    with multiprocessing.Pool(a.j) as pool:
        for n, i, rec in pool.imap_unordered(_state, jobs):
            out[n]["truth"][i] = rec
    out = {n: out[n] for n in cases if n in out}
    with open(R.FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(c, separators=(',', ':'))}" for n, c in out.items()) + "\n}\n")
    print(f"wrote {R.FIXTURE}: {os.path.getsize(R.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
