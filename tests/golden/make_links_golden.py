"""Writes tests/golden/links.json from the restatement (links_restate.py) and the generators (links_cases.py).

  hand       cases small enough to work through link_tree.c by hand (test_links_restate.py holds the hand-worked
             figures; here are the texts the restatement gives for them)
  generated  digests of what the restatement gives for the generated files, under every option of the GPU tests
  hot        the comb and the bush of 4096 links on one k-mer: digests, statistics and histograms (the restatement
             needs minutes for the comb's 8 million tree steps, the GPU test compares against these)

Run from the repository root: python tests/golden/make_links_golden.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import links_cases as LC  # noqa: E402
import links_restate as LR  # noqa: E402

QUIRK = "ACGTA 2\nF 1 10 A seq=ACGTAA juncpos=0\nF 2 2 AC seq=ACGTAAGC juncpos=0,2\n"
HAND = {
    "quirk": {"k": 5, "text": QUIRK},
    "quirk_clean5": {"k": 5, "text": QUIRK, "clean": 5},
    "duplicates": {"k": 5, "text": "ACGTA 3\nF 1 200 G seq=ACGTATG juncpos=1\nF 1 200 G seq=ACGTATG juncpos=1\nF 1 7 T seq=ACGTATT juncpos=1\n"},
    "both_orientations": {"k": 5, "text": "ACGTA 3\nR 1 4 C seq=TACGTC juncpos=0\nF 2 3 AC seq=ACGTAAGC juncpos=0,2\nR 2 5 CG seq=TACGTCTTG juncpos=0,3\n"},
    "hist_3x4": {"k": 5, "hist": [3, 4],
                 "text": "ACGTA 3\nF 3 2 ACG seq=ACGTAACTTG juncpos=0,1,4\nF 2 9 AT seq=ACGTAAT juncpos=0,1\nF 1 1 C seq=ACGTAC juncpos=0\n"},
    "limit": {"k": 5, "limit": 1, "text": QUIRK + "CCCCC 1\nF 1 1 A seq=CCCCCA juncpos=0\n"},
}
OPTIONS = {"plain": {}, "clean2": {"clean": 2}, "clean1000": {"clean": 1000}, "hist": {"hist": (6, 100)}, "hist3x4": {"hist": (3, 4)},
           "clean9_hist": {"clean": 9, "hist": (6, 100)}}
GENERATED = [(5, 300), (31, 200), (33, 200)]


def digest(b):
    return hashlib.sha256(b).hexdigest()


def engine_stats(st):
    return {"kmers_read": st["kmers_read"], "kmers_with_links": st["num_trees_with_links"], "links": st["num_links"],
            "link_bytes": st["num_link_bytes"], "tree_links": st["tree_links"], "links_in": st["links_in"]}


def hot(text, cleans):
    cases = []
    for c in cleans:
        ctp, lst, st, hists = LR.links(text, 5, clean=c, hist=(6, 100))
        cases.append({"clean": c, "stats": engine_stats(st), "hists_nonzero": [[d, c_, n] for d, row in enumerate(hists) for c_, n in enumerate(row) if n], "ctp_sha256": digest(ctp), "ctp_bytes": len(ctp),
                      "list_sha256": digest(lst), "list_bytes": len(lst)})
    return {"input_sha256": digest(text), "cases": cases}


def main():
    out = {"hand": {}, "generated": [], "hot": {}}
    for name, c in HAND.items():
        hist = tuple(c["hist"]) if "hist" in c else None
        ctp, lst, st, hists = LR.links(c["text"].encode(), c["k"], clean=c.get("clean"), hist=hist, limit=c.get("limit", 0))
        out["hand"][name] = dict(c, ctp=ctp.decode(), list=lst.decode(), stats=st, hists=hists)
    for k, n in GENERATED:
        text = LC.generated(k, n, seed=k)
        for name, opt in sorted(OPTIONS.items()):
            ctp, lst, st, hists = LR.links(text, k, **opt)
            out["generated"].append({"k": k, "nkmers": n, "seed": k, "option": name, "input_sha256": digest(text), "ctp_sha256": digest(ctp),
                                     "list_sha256": digest(lst), "stats": st})
    out["hot"]["comb"] = dict(hot(LC.comb(4096), [None, 4096]), n=4096)
    out["hot"]["bush"] = dict(hot(LC.bush(6), [None, 100]), depth=6)
    with open(os.path.join(HERE, "links.json"), "w") as f:
        json.dump(out, f, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
