"""What `unitig_stats`, `clean`, `popbubbles`, `unitigs` and `subgraph` refuse, in which words, and which of them build,
reuse, consume or drop the kept decomposition (csrc/mcx_api.hip): the part of the five entries that the byte-for-byte
suites of the commands do not pin.  Everything is observed through the ABI: the return code with mcx_last_error, the
stats, the checksum, and the launch counts of mcx_graph_profile (k_cl_compact runs once per construction of the dense
ids, k_cl_unitig once per full decomposition).

The graph is one k = 31, one-colour genome of 400 bases loaded twice and a copy with one SNP loaded once: 401 k-mers
and one bubble whose weaker branch popbubbles removes.  Intersect mode needs a second colour, so those refusals use an
empty two-colour handle; they return before any kernel runs.

Not tested: "... takes graphs of fewer than 2^31 k-mers": no test builds a graph that large."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402
import mccortex_amd as mcx  # noqa: E402
from mccortex_amd import graph as G  # noqa: E402

pytestmark = pytest.mark.gpu

K = 31
FOREVER = 2**32 - 1
ERR_ARG = "mcx error -1: "


def reads():
    g1 = synth.genome(400, seed=11)
    g2 = g1.copy()
    g2[200] = ord("ACGT"["ACGT".index(chr(g1[200])) ^ 1])
    return np.concatenate([g1, g1, g2]), np.array([0, 400, 800, 1200], dtype=np.uint64)


def load(profile=True):
    g = mcx.Graph(K, 1, 1 << 16)
    g.add_reads(0, *reads())
    g.sync()
    assert g.nkmers == 401
    if profile:
        g.configure("profile", 1)
    return g


def launches(g, name):
    return g.profile().get(name, (0, 0.0))[0]


def keep_everything(g, unitigs=False):
    """a subgraph run seeded with every k-mer of the graph: nothing is removed, the table stays as it is"""
    before = g.checksum()
    bases, offs = reads()
    g.subgraph_begin(unitigs)
    g.subgraph_seed(bases, offs)
    st = g.subgraph_finish(FOREVER, unitigs=unitigs)
    assert st["nkmers_removed"] == 0 and st["nkmers_kept"] == 401 and g.checksum() == before
    return st


@pytest.fixture(scope="module")
def popped():
    """popbubbles' stats on the graph as loaded"""
    g = load(profile=False)
    st = g.pop_bubbles()
    g.close()
    assert st["num_popped"] == 1 and st["nkmers_before"] == 401 and st["nkmers_removed"] == K
    return st


def sink():
    return G.SINK_FN(lambda _ctx, _ptr, _n: 0)


def entries(h, flags=0):
    """the five entries (unitigs in both forms) as calls on the raw handle h"""
    L = mcx.lib()
    arr = G.UnitigsArrays()
    return {
        "unitig_stats": lambda: L.mcx_graph_unitig_stats(h, None),
        "clean": lambda: L.mcx_graph_clean(h, 0, 0, None, None),
        "pop_bubbles": lambda: L.mcx_graph_pop_bubbles(h, -1, -1, -1, None),
        "unitigs": lambda: L.mcx_graph_unitigs(h, 0, flags, sink(), None, None),
        "unitigs_dev": lambda: L.mcx_graph_unitigs_dev(h, C.byref(arr), None),
        "subgraph": lambda: L.mcx_graph_subgraph_begin(h, flags),
    }


def refused(call):
    rc = call()
    assert rc != 0
    return "mcx error %d: %s" % (rc, mcx.lib().mcx_last_error().decode())


def test_intersect_mode_is_refused_in_todays_words():
    g = mcx.Graph(K, 2, 1 << 16)
    g.configure("intersect", 1)
    said = {name: refused(call) for name, call in entries(g.h).items()}
    tail = " does not take a graph in intersect mode"
    assert said == {
        "unitig_stats": ERR_ARG + "clean" + tail,
        "clean": ERR_ARG + "clean" + tail,
        "pop_bubbles": ERR_ARG + "popbubbles" + tail,
        "unitigs": ERR_ARG + "clean" + tail,
        "unitigs_dev": ERR_ARG + "clean" + tail,
        "subgraph": ERR_ARG + "subgraph" + tail,
    }
    # the mode is refused before the flags are looked at, in subgraph; unitigs looks at its flags first
    assert refused(entries(g.h, 8)["subgraph"]) == ERR_ARG + "subgraph" + tail
    assert refused(entries(g.h, 8)["unitigs"]) == ERR_ARG + "unknown unitigs flags 0x8"
    g.close()


def test_a_split_graph_is_refused_in_todays_words():
    g = mcx.Graph(K, 1, 1 << 16, nparts=2, part=0)
    said = {name: refused(call) for name, call in entries(g.h).items()}
    tail = " needs the whole table on one device, not a graph split over devices (unitigs cross shards)"
    for name, text in said.items():
        assert text == ERR_ARG + {"pop_bubbles": "popbubbles", "subgraph": "subgraph"}.get(name, "clean") + tail, name
    g.close()


def test_null_arguments_are_refused_in_todays_words():
    said = {name: refused(call) for name, call in entries(None).items()}
    assert said == {
        "unitig_stats": ERR_ARG + "null graph",
        "clean": ERR_ARG + "null graph",
        "pop_bubbles": ERR_ARG + "null graph",
        "unitigs": ERR_ARG + "null argument",
        "unitigs_dev": ERR_ARG + "null argument",
        "subgraph": ERR_ARG + "null graph",
    }
    g = load(profile=False)
    L = mcx.lib()
    assert refused(lambda: L.mcx_graph_unitigs(g.h, 0, 0, G.SINK_FN(), None, None)) == ERR_ARG + "null argument"
    assert refused(lambda: L.mcx_graph_unitigs_dev(g.h, None, None)) == ERR_ARG + "null argument"
    g.close()


def test_unknown_flags_are_refused_in_todays_words_and_touch_nothing(popped):
    g = load()
    L = mcx.lib()
    g.unitig_stats()
    assert launches(g, "k_cl_compact") == 1
    assert refused(entries(g.h, 8)["subgraph"]) == ERR_ARG + "subgraph: unknown flags 0x8"
    assert refused(entries(g.h, 0x80000004)["subgraph"]) == ERR_ARG + "subgraph: unknown flags 0x80000004"
    assert refused(entries(g.h, 2)["unitigs"]) == ERR_ARG + "unknown unitigs flags 0x2"
    assert refused(lambda: L.mcx_graph_unitigs(g.h, 7, 0, sink(), None, None)) == ERR_ARG + "unknown unitigs format 7"
    assert refused(lambda: L.mcx_graph_unitigs(g.h, 0, 1, sink(), None, None)) == ERR_ARG + "MCX_UNITIGS_POINTS is for MCX_UNITIGS_DOT only"
    # a refused begin opens nothing
    assert refused(lambda: L.mcx_graph_subgraph_finish(g.h, 1, 0, None)) == ERR_ARG + "subgraph: no mcx_graph_subgraph_begin before the finish"
    # ... and the decomposition is still there and current: popbubbles does not build another
    assert g.pop_bubbles() == popped
    assert launches(g, "k_cl_compact") == 1 and launches(g, "k_cl_unitig") == 1
    g.close()


def test_who_reuses_and_who_drops_the_decomposition(popped):
    g = load()
    g.unitig_stats()
    g.unitig_stats()  # always anew
    assert launches(g, "k_cl_compact") == 2 and launches(g, "k_cl_unitig") == 2
    stats = {}
    text = g.unitigs("fasta", stats=stats)
    assert stats["num_kmers"] == 401 and text.count(b">") == stats["num_unitigs"]
    assert launches(g, "k_cl_compact") == 2  # reused, and left in place
    st, _ = g.clean(0, 0)
    assert st["nkmers_removed"] == 0 and launches(g, "k_cl_compact") == 2  # reused
    assert g.pop_bubbles() == popped
    assert launches(g, "k_cl_compact") == 3 and launches(g, "k_cl_unitig") == 3  # clean had dropped it
    g.unitigs("gfa")
    assert launches(g, "k_cl_compact") == 4  # popbubbles pruned: it had dropped it too
    g.close()


def test_plain_subgraph_leaves_no_decomposition(popped):
    g = load()
    keep_everything(g)
    assert launches(g, "k_cl_compact") == 1 and launches(g, "k_cl_unitig") == 0  # the dense ids alone
    assert g.pop_bubbles() == popped
    assert launches(g, "k_cl_compact") == 2 and launches(g, "k_cl_unitig") == 1  # nothing was there to reuse
    g.close()


def test_subgraph_with_unitigs_builds_the_decomposition_and_takes_it_along(popped):
    g = load()
    keep_everything(g, unitigs=True)
    assert launches(g, "k_cl_compact") == 1 and launches(g, "k_cl_unitig") == 1
    assert g.pop_bubbles() == popped
    assert launches(g, "k_cl_compact") == 2 and launches(g, "k_cl_unitig") == 2
    g.close()


@pytest.mark.parametrize("unitigs", [False, True])
def test_subgraph_consumes_a_current_decomposition(popped, unitigs):
    g = load()
    g.unitig_stats()
    keep_everything(g, unitigs)
    assert launches(g, "k_cl_compact") == 1 and launches(g, "k_cl_unitig") == 1  # its ids were the decomposition's
    assert g.pop_bubbles() == popped
    assert launches(g, "k_cl_compact") == 2 and launches(g, "k_cl_unitig") == 2  # the table is as it was, the decomposition gone
    g.close()
