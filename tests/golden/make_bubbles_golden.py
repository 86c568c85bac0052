"""Writes tests/golden/bubbles.json: the text and stats that the restatement (tests/bubbles_restate.py) gives for every
case of tests/bubbles_cases.py, and the DNA strings of the reference's own unit test of its bubble caller
(src/tests/bubble_caller_tests.c) as data: sequences (one colour each), k, the two flanks and the expected alleles.

    python tests/golden/make_bubbles_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bubbles_cases as BC  # noqa: E402

SEQS0 = ["AGGGATAAAACTCTGTACTGGATCTCCCT", "AGGGATAAAACTCTcTACTGGATCTCCCT"]
SEQS1 = ["CCCGTAGGTAAGGGCGTTAGTGCAAGGCCACATTGGGACACGAGTTGATA", "CCCGTAGGTAAGtGCGTTAGTGCAAGGCCACATTGGGACACGAGTTGATA",
         "CCCGTAGGTAAGGGCGTTAGTGCAAGGCCACtTTGGGACACGAGTTGATA"]
UNIT_TEST = {"k": 11, "max_allele": 100, "max_flank": 100, "calls": [
    {"seqs": SEQS0, "flank5p": "AGGGATAAAACTCT", "flank3p": "TACTGGATCTCCCT", "alleles": ["ATAAAACTCTGTACTGGATCT", "ATAAAACTCTcTACTGGATCT"]},
    {"seqs": SEQS1, "flank5p": "CCCGTAGGTAAG", "flank3p": "GCGTTAGTGCAAGGCCAC", "alleles": ["CGTAGGTAAGGGCGTTAGTGC", "CGTAGGTAAGtGCGTTAGTGC"]},
    {"seqs": SEQS1, "flank5p": "GCGTTAGTGCAAGGCCAC", "flank3p": "TTGGGACACGAGTTGATA", "alleles": ["GCAAGGCCACATTGGGACACG", "GCAAGGCCACtTTGGGACACG"]},
    {"seqs": SEQS1, "flank5p": "GTGGCCTTGCACTAACGC", "flank3p": "CTTACCTACGGG", "alleles": ["GCACTAACGCCCTTACCTACG", "GCACTAACGCaCTTACCTACG"]},
    {"seqs": SEQS1, "flank5p": "TATCAACTCGTGTCCCAA", "flank3p": "GTGGCCTTGCACTAACGC", "alleles": ["CGTGTCCCAATGTGGCCTTGC", "CGTGTCCCAAaGTGGCCTTGC"]},
]}


def plain(case):
    _, text, stats, _ = BC.run(case)
    return {"text": text, "stats": stats}


if __name__ == "__main__":
    out = {"cases": {c["name"]: plain(c) for c in BC.cases()}, "unit_test": UNIT_TEST}
    with open(os.path.join(HERE, "bubbles.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
