"""Writes tests/golden/breakpoints.json: the text and stats that the restatement (tests/breakpoints_restate.py) gives for
every case of tests/breakpoints_cases.py and for the breakpoint1 fixture (tests/golden/breakpoint1_ref.fa and
breakpoint1_sample.fa: the sequences that the reference's tests/breakpoint/breakpoint1 writes, as data) at k = 11 and
min_ref 5.

    python tests/golden/make_breakpoints_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import breakpoints_cases as BC  # noqa: E402
import breakpoints_restate as B  # noqa: E402
import clean_restate as R  # noqa: E402


def fasta(name):
    names, seqs = [], []
    with open(os.path.join(HERE, name)) as f:
        for line in f:
            if line.startswith(">"):
                names.append(line[1:].strip())
                seqs.append("")
            else:
                seqs[-1] += line.strip()
    return names, seqs


def fixture1(ref_edges=True):
    names, ref = fasta("breakpoint1_ref.fa")
    _, sample = fasta("breakpoint1_sample.fa")
    graph = R.build([[s.upper() for s in sample], []], 11)
    return B.call(graph, 11, 2, ref, names, 5, 1000, ref_edges)


def plain(res):
    return {"text": res[1], "stats": res[2]}


if __name__ == "__main__":
    out = {"cases": {c["name"]: plain(BC.run(c)) for c in BC.cases()}, "breakpoint1": plain(fixture1())}
    with open(os.path.join(HERE, "breakpoints.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
