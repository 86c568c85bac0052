"""`coverage`, `correct` and `thread` with small staging buffers: MCX_STAGE_BYTES = 1024 makes a staging buffer of 1040
bytes (the packed layout of mcx_graph_add_reads, the default), so the stand-alone chunks of the read commands hold 640
stream bytes (40 reads at the most) and a finished text goes to its sink 1040 bytes at a time.  The reads here spread
over many chunks and one goes in three pieces; every text makes several rounds on both staging buffers.  The bytes, the
offsets and the stats are compared with the restatements by the checkers of test_gpu_coverage.py, test_gpu_correct.py
and test_gpu_thread.py.  (`reads` refuses buffers of less than 1136 bytes and is not part of this.)
MCX_STAGE_BYTES is read once per process, so the device part runs in a child process (this file, run as a script)."""
import functools
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import correct_cases as CC  # noqa: E402
import correct_restate as X  # noqa: E402
import thread_cases as TC  # noqa: E402

STAGE, CHUNK = 1040, 640  # bytes of a staging buffer; stream bytes of a stand-alone chunk in it
KS = (31, 95)


def aimed_and_long(reads, aimed):
    """the reads aimed at a structure, and behind them the three 600-base reads made one (an N between them) so that the
    second one's error at base 250 lies in what the first two pieces share"""
    lo = aimed["long"][0]
    long_ = reads[lo][:374] + "N" + reads[lo + 1] + "N" + reads[lo + 2]
    return list(reads[min(a for a, _ in aimed.values()):]) + [long_]


def check_sizes(reads, texts):
    assert sum(len(s) + 1 for s in reads) > 4 * CHUNK and max(len(s) for s in reads) > 2 * CHUNK
    assert all(len(t) > 4 * STAGE for t in texts), [len(t) for t in texts]


@functools.lru_cache(maxsize=None)
def coverage_case(k):
    from test_gpu_coverage import Expect, case_seams
    graph, reads = case_seams(k, 1)
    return graph, Expect(graph, k, 1, reads)


@functools.lru_cache(maxsize=None)
def correct_case(k):
    graph, colour, reads, quals, aimed = CC.case(k, 1)
    reads = aimed_and_long(reads, aimed)
    quals = ["".join(chr(33 + (5 * i + j) % 60) for j in range(len(s))) for i, s in enumerate(reads)]
    return graph, colour, reads, quals, X.batch(graph, k, reads, quals, colour=colour, two_way=True)


@functools.lru_cache(maxsize=None)
def thread_case(k):
    graph, reads, aimed = TC.case(k)
    reads = aimed_and_long(reads, aimed)
    return graph, reads, TC.store(k).thread(reads)


def child(k):
    sys.path.insert(0, ROOT)
    import test_gpu_correct as GC
    import test_gpu_coverage as GV
    import test_gpu_thread as GT
    graph, exp = coverage_case(k)
    g = GV.load(graph, k, 1)
    GV.check_text(g, exp, "small staging buffers", combos=((True, True),))
    g.close()
    graph, colour, reads, quals, want = correct_case(k)
    g = GC.load(graph, k, 1)
    GC.check(g, reads, quals, want, "small staging buffers", colour=colour, two_way=True)
    g.close()
    graph, reads, want = thread_case(k)
    g = GT.load(graph, k)
    GT.same(g, want, "small staging buffers", GT.thread(g, reads))
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_texts_over_small_staging_buffers(mcx, k):
    graph, exp = coverage_case(k)
    check_sizes(exp.reads, ["".join(exp.lines[True, True])])
    graph, colour, reads, quals, (text, off, stats) = correct_case(k)
    check_sizes(reads, [text])
    rec = text[off[-2]:off[-1]].decode()  # (the sequence, then as many quality bytes)
    assert rec[:len(rec) // 2].upper() != reads[-1].upper() and stats["gaps_filled"] >= 3, "the read in pieces is corrected"
    graph, reads, want = thread_case(k)
    check_sizes(reads, [want.text(seq=True), want.text(seq=False)])
    env = dict(os.environ, MCX_STAGE_BYTES="1024")
    env.pop("MCX_PACKED", None)  # the default layout, whose buffers are the smaller ones
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(k)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    print(p.stdout.decode(errors="replace")[-2000:])
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]


if __name__ == "__main__":
    child(int(sys.argv[1]))
