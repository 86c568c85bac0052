"""Whole transcripts of the host commands: exit status, stdout, every stderr line in order, and the files left behind,
compared with golden/cli_transcripts.json (recorded by golden/make_cli_transcripts.py from this project's binaries).
The other CLI tests look for substrings; these catch a line that moved, changed or went missing.

stderr is normalised by stripping the `[<date>-<run tag>] ` stamp and replacing the case's own directory with <TMP>;
MASKS lists the only fields that differ between two runs of the same binary.  To keep the golden file small, the usage
text that ends a refused command line is held as its first line, its length and its SHA-256 (the other CLI tests spell
its lines out), and of the files only those that the command created, changed or removed are listed.  The cases not marked gpu run with the
device hidden from the child, so they end at "No MI355X / HIP device found" on every machine."""
import gzip
import hashlib
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
GOLDEN_JSON = os.path.join(GOLD, "cli_transcripts.json")
TOKEN = "<TMP>"
STAMP = re.compile(r"^\[\d\d \w{3} \d{4} \d\d:\d\d:\d\d-[A-Z0-9]{3}\] ")
# the wall time that main() prints after a successful command
MASKS = [(re.compile(r"^\[time\] \d+\.\d\d seconds$"), "[time] <secs> seconds")]
CHILD_TIMEOUT = 60


def sandbox(d):
    """what every case finds in its directory"""
    for f in ("tiny_k31.ctx", "tiny_k5.ctx"):
        shutil.copy(os.path.join(GOLD, f), os.path.join(d, f))
    reads = open(os.path.join(GOLD, "tiny_k31.colour0.txt")).read().split("\n")
    with open(os.path.join(d, "in.fa"), "w") as f:
        f.write("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads[:4])))
    with open(os.path.join(d, "seed.fa"), "w") as f:
        f.write(">seed\n%s\n" % reads[1][20:80])
    for f in ("exists.ctx", "exists.txt", "exists.fq.gz"):
        with open(os.path.join(d, f), "wb") as fh:
            fh.write(b"keep")


def files_in(d):
    out = {}
    for base, _, fs in os.walk(d):
        for f in fs:
            p = os.path.join(base, f)
            data = open(p, "rb").read()
            if f.endswith(".gz") and data[:2] == b"\x1f\x8b":
                data = gzip.decompress(data)
            out[os.path.relpath(p, d)] = hashlib.sha256(data).hexdigest()[:16]
    return out


def fold_usage(lines):
    """[..., "usage: mccortex31 clean ...", <the rest of the usage text>] -> [..., "usage: ...", "<N more lines, sha256 X>"]"""
    at = [i for i, line in enumerate(lines) if line.startswith("usage: ")]
    if not at or len(lines) - at[0] < 4:
        return lines
    rest = lines[at[0] + 1:]
    return lines[:at[0] + 1] + ["<%d more lines, sha256 %s>" % (len(rest), hashlib.sha256("\n".join(rest).encode()).hexdigest()[:16])]


def transcript(d, maxk, args, hide_device):
    """runs mccortex<maxk> in the sandbox d; None in place of the status when the child was killed at the time limit"""
    env = dict(os.environ)
    env.pop("MCX_TIMING", None)
    if hide_device:
        env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = "-1"
    name = "mccortex%d" % maxk
    argv = [name] + [a.replace("{T}", d) for a in args]
    before = files_in(d)
    try:
        p = subprocess.run(argv, executable=os.path.join(BIN, name), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=env, cwd=d, timeout=CHILD_TIMEOUT)
        rc, out, err = p.returncode, p.stdout, p.stderr
    except subprocess.TimeoutExpired as e:
        rc, out, err = None, e.stdout or b"", e.stderr or b""
    lines = []
    for line in err.decode(errors="replace").replace(d, TOKEN).split("\n"):
        line = STAMP.sub("", line)
        for rx, to in MASKS:
            line = rx.sub(to, line)
        lines.append(line)
    try:
        text = out.decode("ascii")
        stdout = text.replace(d, TOKEN) if len(text) <= 4096 else None
    except UnicodeDecodeError:
        stdout = None
    if stdout is None:
        stdout = {"sha256": hashlib.sha256(out).hexdigest()[:16], "bytes": len(out)}
    after = files_in(d)
    files = {f: after.get(f) for f in sorted(set(before) | set(after)) if before.get(f) != after.get(f)}  # None: removed
    return {"rc": rc, "stdout": stdout, "stderr": fold_usage(lines), "files": files}


# ---- the cases: (name, MAXK, arguments); {T} is the case's directory ----------------------------------------------
G31, G5 = "{T}/tiny_k31.ctx", "{T}/tiny_k5.ctx"
# a complete command line of each command, and where in it options are inserted
FULL = {
    "build": (["build"], ["-k", "31", "--sample", "s", "--seq", "{T}/in.fa", "{T}/out.ctx"]),
    "sort": (["sort"], ["-o", "{T}/out.ctx", G31]),
    "index": (["index"], ["-o", "{T}/out.idx", G31]),
    "inferedges": (["inferedges"], ["-o", "{T}/out.ctx", G31]),
    "clean": (["clean"], ["-o", "{T}/out.ctx", G31]),
    "popbubbles": (["popbubbles"], ["-o", "{T}/out.ctx", G31]),
    "subgraph": (["subgraph", "--seq", "{T}/seed.fa"], ["-o", "{T}/out.ctx", G31]),
    "unitigs": (["unitigs"], ["-o", "{T}/out.txt", G31]),
    "reads": (["reads", "--seq", "{T}/in.fa:{T}/hits"], [G31]),
    "hashtest": (["hashtest", "-k", "31"], ["1000"]),
}
# the options of the issue's list that each command has; the twice-cases repeat the option with these values
HAS = {
    "build": "mntf", "sort": "mnof", "index": "of", "inferedges": "mntof", "clean": "mntof", "popbubbles": "mntof",
    "subgraph": "mntof", "unitigs": "mntof", "reads": "mntf", "hashtest": "mnt",
}
TWICE = {"m": ["-m", "1G", "-m", "2G"], "n": ["-n", "1M", "--nkmers", "2M"], "t": ["-t", "2", "--threads", "3"],
         "o": ["-o", "{T}/a.out", "--out", "{T}/b.out"], "f": ["-f", "--force"]}
BAD = {"m": ["-m", "0"], "n": ["-n", "banana"], "t": ["-t", "0"]}


def with_opts(cmd, opts):
    head, rest = FULL[cmd]
    if "-o" in opts:  # the case brings its own
        rest = [a for i, a in enumerate(rest) if not (a == "-o" or (i and rest[i - 1] == "-o"))]
    return head + opts + rest


def cpu_cases():
    cases = [("dispatch.noargs", 31, []), ("dispatch.help", 31, ["-h"]), ("dispatch.unknown", 31, ["view", "x.ctx"]),
             ("dispatch.quiet", 31, ["-q", "unitigs", G31])]
    for cmd in FULL:
        for maxk in (31, 63, 95, 127):
            cases.append(("%s.help.k%d" % (cmd, maxk), maxk, [cmd, "-h"]))
        cases.append((cmd + ".noargs", 31, [cmd]))
        for o in HAS[cmd]:
            cases.append(("%s.twice.%s" % (cmd, o), 31, with_opts(cmd, TWICE[o])))
            if o in BAD:
                cases.append(("%s.bad.%s" % (cmd, o), 31, with_opts(cmd, BAD[o])))
        cases.append((cmd + ".device.x", 31, with_opts(cmd, ["--device", "x"])))
        cases.append((cmd + ".device.twice", 31, with_opts(cmd, ["--device", "0", "--device", "0"])))
        cases.append((cmd + ".unknown", 31, with_opts(cmd, ["--nosuchoption"])))
        cases.append((cmd + ".refusal", 31, with_opts(cmd, [])))
        if cmd not in ("build", "hashtest"):
            head, rest = FULL[cmd]
            cases.append((cmd + ".nograph", 31, head + rest[:-1]))
            cases.append((cmd + ".missing", 31, head + rest[:-1] + ["{T}/missing.ctx"]))
            cases.append((cmd + ".kmismatch", 31, head + rest + [G5]))
            cases.append((cmd + ".k5.refusal", 31, head + rest[:-1] + [G5]))
    ex = "{T}/exists.ctx"
    cases += [
        # an output that exists, without --force
        ("sort.exists", 31, ["sort", "-o", ex, G31]),
        ("index.exists", 31, ["index", "-o", ex, G31]),
        ("inferedges.exists", 31, ["inferedges", "-o", ex, G31]),
        ("clean.exists", 31, ["clean", "-o", ex, G31]),
        ("popbubbles.exists", 31, ["popbubbles", "-o", ex, G31]),
        ("subgraph.exists", 31, ["subgraph", "--seq", "{T}/seed.fa", "-o", ex, G31]),
        ("unitigs.exists", 31, ["unitigs", "-o", "{T}/exists.txt", G31]),
        ("reads.exists", 31, ["reads", "--seq", "{T}/in.fa:{T}/new", "--seq", "{T}/in.fa:{T}/exists", G31]),
        ("clean.exists.force", 31, ["clean", "-f", "-o", ex, G31]),
        ("popbubbles.exists.force", 31, ["popbubbles", "-f", "-o", ex, G31]),
        ("unitigs.exists.force", 31, ["unitigs", "-f", "-o", "{T}/exists.txt", G31]),
        # build
        ("build.missing.seq", 31, ["build", "-k", "31", "--sample", "s", "--seq", "{T}/missing.fa", "{T}/out.ctx"]),
        ("build.missing.graph", 31, ["build", "-k", "31", "--graph", "{T}/missing.ctx", "{T}/out.ctx"]),
        ("build.kmismatch", 31, ["build", "-k", "31", "--graph", G5, "--sample", "s", "--seq", "{T}/in.fa", "{T}/out.ctx"]),
        ("build.graph.filter", 31, ["build", "-k", "31", "--graph", "0:{T}/tiny_k31.ctx:1", "--sample", "s", "--seq", "{T}/in.fa",
                                    "{T}/out.ctx"]),
        ("build.intersect", 31, ["build", "-k", "31", "--intersect", G31, "--sample", "s", "--seq", "{T}/in.fa", "{T}/out.ctx"]),
        ("build.sort.twice", 31, ["build", "-S", "--sort", "-k", "31", "--sample", "s", "--seq", "{T}/in.fa", "{T}/out.ctx"]),
        ("build.nokmer", 31, ["build", "--sample", "s", "--seq", "{T}/in.fa", "{T}/out.ctx"]),
        ("build.stdout", 31, ["build", "-k", "31", "--sample", "s", "--seq", "{T}/in.fa", "-"]),
        # sort, index
        ("sort.inplace", 31, ["sort", G31]),
        ("sort.filter", 31, ["sort", "-o", "{T}/out.ctx", G31 + ":0"]),
        ("sort.small.memory", 31, ["sort", "-m", "1K", "-o", "{T}/out.ctx", G31]),
        ("index.stdout", 31, ["index", G5]),
        ("index.block.kmers", 31, ["index", "-b", "100", "-o", "{T}/out.idx", G5]),
        ("index.block.zero", 31, ["index", "-s", "0", G5]),
        ("index.block.both", 31, ["index", "-s", "1000", "-b", "10", G5]),
        ("index.block.twice", 31, ["index", "-b", "10", "-b", "10", G5]),
        # inferedges: -t, -A and -P may be repeated; nthreads stays 0
        ("inferedges.inplace", 31, ["inferedges", G31]),
        ("inferedges.all.twice", 31, ["inferedges", "-A", "--all", G31]),
        ("inferedges.pop.twice", 31, ["inferedges", "-P", "--pop", "-o", "{T}/out.ctx", G31]),
        ("inferedges.all.pop", 31, ["inferedges", "-A", "-P", G31]),
        ("inferedges.filter", 31, ["inferedges", G31 + ":0"]),
        ("inferedges.stdout", 31, ["inferedges", "-o", "-", G31]),
        ("inferedges.nkmers.small", 31, ["inferedges", "-n", "16", G31]),
        # clean
        ("clean.ncols.twice", 31, ["clean", "-N", "1", "--ncols", "2", "-o", "{T}/out.ctx", G31]),
        ("clean.ncols.more", 31, ["clean", "-N", "5", "-o", "{T}/out.ctx", G31]),
        ("clean.tips.twice", 31, ["clean", "-T", "-T", "-o", "{T}/out.ctx", G31]),
        ("clean.unitigs.twice", 31, ["clean", "-U3", "--unitigs=4", "-o", "{T}/out.ctx", G31]),
        ("clean.fallback.twice", 31, ["clean", "-B", "2", "-B", "3", "-o", "{T}/out.ctx", G31]),
        ("clean.tips.noout", 31, ["clean", "--tips=10", G31]),
        ("clean.stats", 31, ["clean", "--covg-before", "{T}/covg.csv", "--len-before", "{T}/len.csv", G31, G31]),
        ("clean.stats.after", 31, ["clean", "--covg-after", "{T}/covg.csv", "-B", "2", G31]),
        ("clean.sort.two.files", 31, ["clean", "-S", "-T", "-U", "-o", "{T}/out.ctx", G31, G31 + ":1"]),
        ("clean.stdout", 31, ["clean", "-o", "-", G31]),
        ("clean.memory.small", 31, ["clean", "-m", "1K", "-o", "{T}/out.ctx", G31]),
        ("clean.nkmers.small", 31, ["clean", "-n", "16", "-o", "{T}/out.ctx", G31]),
        # popbubbles, subgraph
        ("popbubbles.limits", 31, ["popbubbles", "-C", "3", "-L", "20", "-D", "2", "-S", "-o", "{T}/out.ctx", G31]),
        ("popbubbles.covg.twice", 31, ["popbubbles", "-C", "3", "--max-covg", "4", G31]),
        ("popbubbles.sort.twice", 31, ["popbubbles", "-S", "--sort", G31]),
        ("popbubbles.limit.bad", 31, ["popbubbles", "-L", "x", G31]),
        ("popbubbles.memory.small", 31, ["popbubbles", "-m", "1K", G31]),
        ("popbubbles.stdout", 31, ["popbubbles", G31]),
        ("subgraph.noseed", 31, ["subgraph", "-o", "{T}/out.ctx", G31]),
        ("subgraph.seed.missing", 31, ["subgraph", "--seed", "{T}/missing.fa", G31]),
        ("subgraph.ncols.twice", 31, ["subgraph", "--seq", "{T}/seed.fa", "-N", "1", "--ncols", "2", G31]),
        ("subgraph.dist.twice", 31, ["subgraph", "--seq", "{T}/seed.fa", "-d", "1", "--dist", "2", G31]),
        ("subgraph.sort.invert.unitigs", 31, ["subgraph", "-1", "{T}/seed.fa", "--sort", "-v", "-U", "-d", "3", "-o", "{T}/out.ctx", G31, G31]),
        ("subgraph.memory.small", 31, ["subgraph", "--seq", "{T}/seed.fa", "-m", "1K", G31]),
        # unitigs, reads
        ("unitigs.gfa.dot", 31, ["unitigs", "--gfa", "--dot", G31]),
        ("unitigs.points.fasta", 31, ["unitigs", "-P", G31]),
        ("unitigs.points.gfa", 31, ["unitigs", "-P", "-g", G31]),
        ("unitigs.stdout.two.files", 31, ["unitigs", "--dot", "--points", G31, G31 + ":0"]),
        ("unitigs.memory.small", 31, ["unitigs", "-m", "1K", G31]),
        ("reads.notask", 31, ["reads", G31]),
        ("reads.format.bad", 31, ["reads", "--seq", "{T}/in.fa:{T}/hits", "-F", "SAM", G31]),
        ("reads.format.twice", 31, ["reads", "--seq", "{T}/in.fa:{T}/hits", "-F", "fa", "-F", "fq", G31]),
        ("reads.invert.twice", 31, ["reads", "--seq", "{T}/in.fa:{T}/hits", "-v", "--invert", G31]),
        ("reads.task.bad", 31, ["reads", "--seq", "{T}/in.fa", G31]),
        ("reads.three.tasks", 31, ["reads", "-F", "fa", "--seq", "{T}/in.fa:{T}/deep/a", "--seq2", "{T}/in.fa:{T}/in.fa:{T}/b", "--seqi",
                                   "{T}/in.fa:{T}/c", G31, G31]),
        ("reads.memory.small", 31, ["reads", "--seq", "{T}/in.fa:{T}/hits", "-m", "1K", G31]),
        ("reads.nkmers.small", 31, ["reads", "--seq", "{T}/in.fa:{T}/hits", "--seq", "{T}/in.fa:{T}/more", "-n", "16", G31]),
        # hashtest
        ("hashtest.nokmer", 31, ["hashtest", "1000"]),
        ("hashtest.kmer.even", 31, ["hashtest", "-k", "30", "1000"]),
        ("hashtest.kmer.twice", 31, ["hashtest", "-k", "31", "-k", "31", "1000"]),
        ("hashtest.kmer.wide", 31, ["hashtest", "-k", "33", "1000"]),
        ("hashtest.noops", 31, ["hashtest", "-k", "31"]),
        ("hashtest.ops.bad", 31, ["hashtest", "-k", "31", "lots"]),
        ("hashtest.func.twice", 31, ["hashtest", "-k", "31", "-F", "--func-only", "1000"]),
        ("hashtest.func.refusal", 31, ["hashtest", "-k", "31", "-F", "1000"]),
        # the wider binaries get as far as the narrow one
        ("clean.k63.toosmall", 63, ["clean", "-o", "{T}/out.ctx", G31]),
        ("unitigs.k127.toosmall", 127, ["unitigs", G5]),
    ]
    return cases


def gpu_cases():
    """(graphs are written with --sort: the order of an unsorted export is the table's, which two runs need not share)"""
    return [
        ("clean.out", 31, ["clean", "--sort", "--fallback", "2", "-o", "{T}/out.ctx", G31]),
        ("clean.stats.covg.before", 31, ["clean", "--covg-before", "{T}/covg.csv", "-B", "2", G31]),
        ("clean.k5.two.files.sorted", 31, ["clean", "-S", "-T8", "-U2", "-C", "{T}/after.csv", "-L", "-", "-o", "{T}/out.ctx", G5, G5]),
        ("popbubbles.sorted", 31, ["popbubbles", "-S", "-o", "{T}/out.ctx", G31]),
        ("popbubbles.k5.stdout", 31, ["popbubbles", "--sort", "-L", "10", G5]),
        ("subgraph.seq", 31, ["subgraph", "--seq", "{T}/seed.fa", "--dist", "2", "--sort", "-o", "{T}/out.ctx", G31]),
        ("unitigs.gfa", 31, ["unitigs", "--gfa", G31]),
        ("unitigs.k5.fasta.file", 31, ["unitigs", "-o", "{T}/out.fa", G5]),
        ("reads.seq", 31, ["reads", "--seq", "{T}/in.fa:{T}/hits", G31]),
        ("inferedges.out", 31, ["inferedges", "-o", "{T}/out.ctx", G31]),
        ("inferedges.inplace", 31, ["inferedges", G31]),
        ("build.graph.filter", 31, ["build", "-S", "-k", "31", "--graph", "0:{T}/tiny_k31.ctx:1", "--sample", "s", "--seq", "{T}/in.fa",
                                    "{T}/out.ctx"]),
        ("sort.out", 31, ["sort", "-o", "{T}/out.ctx", G31]),
    ]


CPU_CASES, GPU_CASES = cpu_cases(), gpu_cases()
assert len({c[0] for c in CPU_CASES}) == len(CPU_CASES) and len({c[0] for c in GPU_CASES}) == len(GPU_CASES)


def describe(got, exp):
    """the first difference, for the assertion message"""
    for key in ("rc", "stdout", "files"):
        if got[key] != exp[key]:
            return "%s: %r, recorded %r" % (key, got[key], exp[key])
    for i, (a, b) in enumerate(zip(got["stderr"], exp["stderr"])):
        if a != b:
            return "stderr line %d: %r, recorded %r" % (i, a, b)
    return "stderr has %d lines, recorded %d: %r" % (len(got["stderr"]), len(exp["stderr"]), (got["stderr"] + exp["stderr"])[-1])


@pytest.fixture(scope="module")
def golden(mcx):
    return json.load(open(GOLDEN_JSON))


@pytest.mark.parametrize("name,maxk,args", CPU_CASES, ids=[c[0] for c in CPU_CASES])
def test_transcript_without_device(golden, tmp_path, name, maxk, args):
    d = str(tmp_path)
    sandbox(d)
    got = transcript(d, maxk, args, hide_device=True)
    assert got == golden["cpu"][name], describe(got, golden["cpu"][name])
    if name.endswith(".exists"):  # refused, and the file in the way is as it was
        assert got["rc"] == 1 and all(open(os.path.join(d, f), "rb").read() == b"keep" for f in ("exists.ctx", "exists.txt", "exists.fq.gz"))
    if name.startswith("reads."):  # whatever stopped the command, none of its outputs stays behind
        assert got["rc"] == 1 and got["files"] == {}, got["files"]
    if name.endswith("refusal") and not name.startswith("index."):  # (index works without a device)
        assert got["rc"] == 1 and any(line.startswith("Fatal Error: No MI355X / HIP device found") for line in got["stderr"])


stopped = []  # the first child that ended on a signal or at the time limit: nothing runs on the device after it


@pytest.mark.gpu
@pytest.mark.parametrize("name,maxk,args", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_transcript_on_device(golden, tmp_path, name, maxk, args):
    assert not stopped, "not run: %s ended with %s" % tuple(stopped[0])
    d = str(tmp_path)
    sandbox(d)
    got = transcript(d, maxk, args, hide_device=False)
    if got["rc"] is None or got["rc"] < 0:
        stopped.append((name, "the time limit" if got["rc"] is None else "signal %d" % -got["rc"]))
    assert got["rc"] == 0, got["stderr"]
    assert got == golden["gpu"][name], describe(got, golden["gpu"][name])
