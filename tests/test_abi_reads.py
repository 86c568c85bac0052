"""CPU tests of the `reads` part of the boundary: mcx_touch_stats as include/mcx_gpu.h declares it against its ctypes
mirror, and the two entries' argument checks that need no device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_touch_stats_layout(mcx):
    src = open(os.path.join(ROOT, "include", "mcx_gpu.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} mcx_touch_stats;", src)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("uint64_t "), decl
            fields += [f.strip() for f in decl[len("uint64_t "):].split(",")]
    assert fields == ["num_reads", "num_reads_hit", "num_kmers", "num_kmers_found"]
    assert [n for n, _ in mcx.TouchStats._fields_] == fields and all(t is C.c_uint64 for _, t in mcx.TouchStats._fields_)
    assert C.sizeof(mcx.TouchStats) == 32
    st = mcx.TouchStats()
    assert st.as_dict() == dict.fromkeys(fields, 0)


def test_null_handle_is_an_argument_error(mcx):
    L = mcx.lib()
    hit = (C.c_uint8 * 4)()
    assert L.mcx_graph_reads_touch(None, None, None, 0, hit, None) == -1
    assert b"null graph" in L.mcx_last_error()
    assert L.mcx_graph_reads_touch_stream_dev(None, None, 0, None, 0, None) == -1
    assert b"null graph" in L.mcx_last_error()
