#!/usr/bin/env python3
"""Records golden/cli_transcripts.json for tests/test_cli_transcripts.py from the binaries under mccortex_amd/bin
(run from a checkout of the commit whose behaviour is to be pinned, after build()).

    python tests/golden/make_cli_transcripts.py          the cases that need no device
    python tests/golden/make_cli_transcripts.py --gpu    the cases that run on the MI355X as well
    ... --only clean.out,sort.out                        these cases alone, the others keep their recordings

Every case is recorded twice; a case whose two recordings differ is reported and makes the script fail: the field that
varies needs a mask in the test's MASKS.  Sections that are not recorded keep what the file held."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_cli_transcripts as T  # noqa: E402


def record(cases, hide_device, old):
    out, bad = {}, 0
    only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
    for name, maxk, args in cases:
        if only and name not in only:
            out[name] = old[name]
            continue
        two = []
        for _ in range(2):
            with tempfile.TemporaryDirectory() as d:
                d = os.path.realpath(d)
                T.sandbox(d)
                two.append(T.transcript(d, maxk, args, hide_device))
            if two[-1]["rc"] is None or two[-1]["rc"] < 0:
                sys.exit("%s: child ended with %r\n%s" % (name, two[-1]["rc"], "\n".join(two[-1]["stderr"])))
        if two[0] != two[1]:
            print("VARIES %s: %s" % (name, T.describe(two[0], two[1])))
            bad += 1
        out[name] = two[0]
    return out, bad


if __name__ == "__main__":
    gold = json.load(open(T.GOLDEN_JSON)) if os.path.exists(T.GOLDEN_JSON) else {}
    gold["cpu"], bad = record(T.CPU_CASES, True, gold.get("cpu"))
    if "--gpu" in sys.argv[1:]:
        gold["gpu"], bad_gpu = record(T.GPU_CASES, False, gold.get("gpu"))
        bad += bad_gpu
    dest = sys.argv[sys.argv.index("--to") + 1] if "--to" in sys.argv else T.GOLDEN_JSON
    with open(dest, "w") as f:  # one line per case
        f.write("{\n" + ",\n".join('"%s": {\n%s\n}' % (sec, ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True))
                                                                     for k, v in sorted(gold[sec].items())))
                                   for sec in sorted(gold)) + "\n}\n")
    print("%d cpu, %d gpu transcripts in %s" % (len(gold["cpu"]), len(gold.get("gpu", {})), dest))
    sys.exit(1 if bad else 0)
