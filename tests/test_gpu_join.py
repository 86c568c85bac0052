"""`join` on the device: the engine (mccortex_amd.Join over mcx_join_*) against the dictionary restatement
(tests/join_restate.py) by exact byte equality of body and counts, and -- for every case without intersection graphs --
against the table route (Graph.add_records per file with the same filter, export(sorted)); then `mccortex<K> join`
against the restatement's header + body.  Inputs are a few hundred to a few thousand records."""
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import join_restate as J  # noqa: E402
from oracle import ctxio  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
U32 = 0xFFFFFFFF


# ---- inputs -----------------------------------------------------------------------------------------------------------
def pool(rng, k, n):
    keys = set()
    while len(keys) < n:
        keys.add(rng.getrandbits(2 * k))
    return sorted(keys)


def rand_file(rng, k, ncols, keys, zero=0.25, big=0.0):
    """a body of the given keys in shuffled order: a quarter of the coverages zero (so some records are dropped whole,
    some have edges without coverage), `big` of them near 2^32"""
    recs = []
    for key in keys:
        cv = [0 if rng.random() < zero else (U32 - rng.randrange(4) if rng.random() < big else rng.randrange(1, 50)) for _ in range(ncols)]
        recs.append((key, cv, [rng.randrange(256) for _ in range(ncols)]))
    rng.shuffle(recs)
    return J.pack(recs, k, ncols)


def engine(mcx, k, ncols, inputs, isecs=(), keep_empty=False, grid=None, out_chunk=None, split=None):
    j = mcx.Join(k, ncols, len(isecs), keep_empty)
    try:
        if grid is not None:
            j.configure("grid", grid)
        if out_chunk is not None:
            j.configure("out_chunk", out_chunk)
        W = ctxio.words_for_k(k)
        for source, (body, nc, filt) in [(r, x) for r, x in enumerate(isecs)] + [(-1, x) for x in inputs]:
            rs = 8 * W + 5 * nc
            n, at, i = len(body) // rs, 0, 0
            if split is None:
                j.add(body, nc, filt, source)
                continue
            while at < n:  # uneven pieces, an empty one among them
                take = min(n - at, split[i % len(split)])
                j.add(body[at * rs:(at + take) * rs], nc, filt, source)
                at, i = at + take, i + 1
        body, st = j.finish()
        return body, st, j.chunks
    finally:
        j.close()


def table(mcx, k, ncols, inputs):
    g = mcx.Graph(k, ncols, 1 << 16)
    try:
        for body, nc, filt in inputs:
            if body:
                g.add_records(body, nc, filt)
        return g.export(sorted_=True)
    finally:
        g.close()


def check(mcx, k, ncols, inputs, isecs=(), keep_empty=False, **knobs):
    exp, exp_st, out = J.join_records(k, ncols, inputs, isecs, keep_empty)
    body, st, chunks = engine(mcx, k, ncols, inputs, isecs, keep_empty, **knobs)
    assert st == exp_st
    assert body == exp
    if not isecs:
        assert table(mcx, k, ncols, inputs) == exp
    return exp_st, out, chunks


# ---- the engine -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [9, 31, 33, 63, 65, 95, 97, 127])
def test_key_widths(mcx, k):
    rng = random.Random(k)
    keys = pool(rng, k, 900)
    inputs = [(rand_file(rng, k, 1, rng.sample(keys, 500)), 1, [(0, c)]) for c in range(3)]
    st, out, _ = check(mcx, k, 3, inputs)
    assert st["recs_kept"] < st["recs_read"] and st["kmers_written"] < st["recs_kept"]  # drops and real runs
    # every kernel's loop more than once, chunk seams inside records; the same records split over uneven calls
    rb = 8 * ctxio.words_for_k(k) + 15
    _, _, chunks = check(mcx, k, 3, inputs, grid=1, out_chunk=3 * rb + 5, split=[7, 0, 301, 64, 1])
    assert len(chunks) > 100 and max(chunks) == 3 * rb + 5


@pytest.mark.parametrize("k", [63, 95, 127])
def test_keys_that_differ_in_one_word(mcx, k):
    W = ctxio.words_for_k(k)
    rng = random.Random(k)
    base = rng.getrandbits(2 * k)
    top_bits = 2 * k - 64 * (W - 1)
    low = [(base & ~0xFFFF) | i for i in range(0, 300)]                                       # the least significant word
    top = [(base & ((1 << 64 * (W - 1)) - 1)) | (i << (64 * (W - 1) + top_bits - 10)) for i in range(300)]  # the top word
    for keys in (low, top, low + top[1:]):
        assert len(set(keys)) == len(keys)
        inputs = [(rand_file(rng, k, 1, rng.sample(keys, 200)), 1, [(0, c)]) for c in range(2)]
        check(mcx, k, 2, inputs)
    words = lambda key: [(key >> (64 * (W - 1 - w))) & (2 ** 64 - 1) for w in range(W)]  # noqa: E731
    assert all(words(a)[:-1] == words(low[0])[:-1] for a in low) and all(words(a)[1:] == words(top[0])[1:] for a in top)


@pytest.mark.parametrize("ncols", [1, 3, 40])
def test_one_colour_files_into_n_colours(mcx, ncols):
    rng = random.Random(ncols)
    keys = pool(rng, 31, 400)
    inputs = [(rand_file(rng, 31, 1, rng.sample(keys, 150)), 1, [(0, c)]) for c in range(ncols)]
    st, out, _ = check(mcx, 31, ncols, inputs)
    if ncols == 40:
        assert max(sum(1 for c in cv if c) for cv, _ in out.values()) > 16
    check(mcx, 31, ncols, inputs, grid=1, out_chunk=1000)


def test_three_colour_file_with_repeated_source_and_target(mcx):
    rng = random.Random(3)
    keys = pool(rng, 33, 500)
    filt = [(0, 0), (0, 1), (2, 1), (1, 1), (2, 3)]
    inputs = [(rand_file(rng, 33, 3, keys, big=0.1), 3, filt), (rand_file(rng, 33, 1, keys[::3]), 1, [(0, 2)])]
    _, out, _ = check(mcx, 33, 4, inputs)
    assert any(cv[1] == U32 for cv, _ in out.values())  # 0 + 2 + 1 into colour 1 saturates within the file's filter
    check(mcx, 33, 4, inputs, grid=1, out_chunk=64)


def test_same_key_in_1_2_and_70_sources(mcx):
    rng = random.Random(70)
    keys = pool(rng, 31, 2000)
    everywhere, twice, rest = keys[0], keys[1], keys[2:]
    inputs = []
    for i in range(70):
        mine = rest[i * 25:(i + 1) * 25] + [everywhere] + ([twice] if i in (3, 44) else [])
        inputs.append((rand_file(rng, 31, 1, mine, zero=0.0), 1, [(0, i % 3)]))
    out = J.join_records(31, 3, inputs)[2]
    total = sum(c[0] for b, _, _ in inputs for key, c, _ in J.parse(b, 31, 1) if key == everywhere)
    assert total >= 70 and sum(out[everywhere][0]) == total and all(out[everywhere][0])
    check(mcx, 31, 3, inputs)            # a run of 70 items: longer than a wave
    check(mcx, 31, 3, inputs, grid=1, out_chunk=23)


def test_same_file_twice_and_saturation(mcx):
    rng = random.Random(5)
    keys = pool(rng, 31, 300)
    a = rand_file(rng, 31, 2, keys, big=0.3)
    b = rand_file(rng, 31, 1, keys, big=0.3)
    _, out, _ = check(mcx, 31, 1, [(a, 2, [(0, 0)]), (a, 2, [(0, 0)])])                      # the same file twice into one colour
    assert any(cv[0] == U32 for cv, _ in out.values()) and any(0 < cv[0] < U32 for cv, _ in out.values())
    ra, rb = {r[0]: r for r in J.parse(a, 31, 2)}, {r[0]: r for r in J.parse(b, 31, 1)}
    assert any(U32 > ra[key][1][0] > 0 and ra[key][1][0] + ra[key][1][1] > U32 for key in keys)   # saturates within one file's filter
    assert any(ra[key][1][0] < 100 and ra[key][1][1] < 100 and ra[key][1][0] + ra[key][1][1] + rb[key][1][0] > U32 for key in keys)  # only across files
    check(mcx, 31, 1, [(a, 2, [(0, 0), (1, 0)]), (b, 1, [(0, 0)])])


def test_empty_inputs(mcx):
    rng = random.Random(6)
    a = rand_file(rng, 65, 1, pool(rng, 65, 100))
    st, _, _ = check(mcx, 65, 2, [(a, 1, [(0, 1)]), (b"", 1, [(0, 0)])])                     # an empty file among the inputs
    assert st["kmers_written"] > 0
    body, st, chunks = engine(mcx, 65, 2, [(b"", 1, [(0, 0)]), (b"", 3, [(2, 1)])])         # all inputs empty
    assert body == b"" and chunks == [] and st == dict.fromkeys(J.STATS, 0)
    nocov = J.pack([(1, [0], [0xFF]), (2, [0], [1])], 65, 1)                                 # records, but none kept
    body, st, _ = engine(mcx, 65, 1, [(nocov, 1, [(0, 0)])])
    assert body == b"" and st["recs_read"] == 2 and st["recs_kept"] == 0


def test_chunk_seams_between_records(mcx):
    rng = random.Random(8)
    inputs = [(rand_file(rng, 31, 1, pool(rng, 31, 700), zero=0.0), 1, [(0, 0)])]
    for chunk in (13, 13 * 64, 13 * 64 + 1, 1, 13 * 700, 1 << 20):
        _, _, chunks = check(mcx, 31, 1, inputs, out_chunk=chunk)
        assert sum(chunks) == 13 * 700 and max(chunks) == min(chunk, 13 * 700) and len(chunks) == -(-13 * 700 // chunk)


# ---- intersections ----------------------------------------------------------------------------------------------------
def isec_case(rng, k=31):
    keys = pool(rng, k, 1200)
    small = rand_file(rng, k, 1, keys[:500])
    big = rand_file(rng, k, 1, keys[200:1000])
    inputs = [(rand_file(rng, k, 1, rng.sample(keys[100:], 700)), 1, [(0, c)]) for c in range(2)]
    return keys, small, big, inputs


def test_intersection_with_one_graph(mcx):
    rng = random.Random(11)
    _, small, _, inputs = isec_case(rng)
    isecs = [(small, 1, [(0, 0)])]
    st, out, _ = check(mcx, 31, 2, inputs, isecs)
    exp, st2, out2 = J.join_records(31, 2, inputs, isecs, keep_empty=True)
    assert st2["kmers_written_no_covg"] > 0 and st["kmers_written"] < st2["kmers_written"] == st2["kmers_intersection"]
    # masks that clear some but not all edge bits
    plain = J.join_records(31, 2, inputs)[2]
    assert any(0 < sum(bin(e).count("1") for e in out[key][1]) < sum(bin(e).count("1") for e in plain[key][1]) for key in out)
    check(mcx, 31, 2, inputs, isecs, keep_empty=True)
    check(mcx, 31, 2, inputs, isecs, keep_empty=True, grid=1, out_chunk=37, split=[100, 3, 0, 999])


def test_intersection_with_two_graphs(mcx):
    rng = random.Random(12)
    _, small, big, inputs = isec_case(rng)
    for keep in (False, True):
        a = check(mcx, 31, 2, inputs, [(small, 1, [(0, 0)]), (big, 1, [(0, 0)])], keep)[1]
        b = check(mcx, 31, 2, inputs, [(big, 1, [(0, 0)]), (small, 1, [(0, 0)])], keep)[1]
        assert sorted(a) == sorted(b) and a != b  # the same keys, another mask: rank 0 decides it
    st = check(mcx, 31, 2, inputs, [(small, 1, [(0, 0)]), (big, 1, [(0, 0)])], True, grid=1, out_chunk=50)[0]
    assert 0 < st["kmers_intersection"] < 500 and st["kmers_written_no_covg"] > 0


def test_intersection_graph_with_a_colour_selection(mcx):
    rng = random.Random(13)
    keys = pool(rng, 63, 600)
    isec2 = rand_file(rng, 63, 2, keys[:400], zero=0.5)
    inputs = [(rand_file(rng, 63, 2, keys[100:]), 2, [(1, 0), (0, 2)])]
    only1 = check(mcx, 63, 3, inputs, [(isec2, 2, [(1, 0)])], True)[0]
    both = check(mcx, 63, 3, inputs, [(isec2, 2, [(0, 0), (1, 0)])], True)[0]
    assert only1["isec_recs_kept"] < both["isec_recs_kept"] < 400
    # 70 intersection graphs: more sources than one presence word holds
    many = [(J.pack([r for r in J.parse(isec2, 63, 2) if r[0] != keys[i]], 63, 2), 2, [(0, 0), (1, 0)]) for i in range(70)]
    st = check(mcx, 63, 3, inputs, many, True)[0]
    assert st["kmers_intersection"] <= both["kmers_intersection"] - 30


def test_argument_errors(mcx):
    with pytest.raises(mcx.McxError):
        mcx.Join(32, 1)
    j = mcx.Join(31, 2, 1)
    rec = J.pack([(1, [1], [1])], 31, 1)
    for filt, source in (([(1, 0)], -1), ([(0, 2)], -1), ([(0, 0)], 1), ([], -1)):
        with pytest.raises(mcx.McxError):
            j.add(rec, 1, filt, source)
    with pytest.raises(mcx.McxError):
        j.configure("nosuchknob", 1)
    j.close()


# ---- the command ------------------------------------------------------------------------------------------------------
def run(maxk, *args):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + [str(a) for a in args], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


def build_samples(tmp, maxk, k, n=3):
    rng = random.Random(k)
    genome = "".join(rng.choice("ACGT") for _ in range(900))
    files = {}
    for i in range(n):
        fa = tmp / ("seq%d.fa" % i)
        fa.write_text("".join(">r%d\n%s\n" % (r, genome[s:s + 200]) for r, s in enumerate(rng.randrange(0, 700) for _ in range(8))))
        out = tmp / ("in%d.ctx" % i)
        rc, _, err = run(maxk, "build", "-q", "-k", k, "--sample", "Sampe%d" % i, "--seq", fa, out)
        assert rc == 0, err
        files[str(out)] = out.read_bytes()
    return files


def join_cli(maxk, files, out, args, isec=(), extra=()):
    cmd = ["join", "-q", "-f", "-o", out] + list(extra)
    for a in isec:
        cmd += ["-i", a]
    rc, so, err = run(maxk, *(cmd + list(args)))
    assert rc == 0 and so == b"", err
    files[str(out)] = out.read_bytes()
    return files[str(out)]


def test_makefile_lines(mcx, tmp_path):
    files = build_samples(tmp_path, 31, 7)
    i0, i1, i2 = sorted(files)
    eight = ["0:" + i0, "1:" + i1, "2:" + i2, "3:" + i0, "3:" + i0, "4:" + i1, "4:" + i2, "5:" + i2]
    merged = tmp_path / "in.ctx"
    got = join_cli(31, files, merged, eight)
    hdr, body, st, ncols = J.join_command(eight, files)
    assert ncols == 6 and st["kmers_written"] > 100 and got == hdr + body
    for n in (1, 2):
        assert join_cli(31, files, tmp_path / ("use%d.ctx" % n), eight, extra=["--ncols", n]) == got
    m = str(merged)
    flat = ["0:%s:1" % m, "0:%s:0" % m, "0:%s:3-3" % m]
    hdr, body, _, ncols = J.join_command(flat, files)
    assert ncols == 1 and join_cli(31, files, tmp_path / "flatten013.ctx", flat) == hdr + body
    gaps = ["1:%s:0" % m, "0:%s:1" % m, "4:%s:3" % m]
    hdr, body, _, ncols = J.join_command(gaps, files)
    assert ncols == 5
    g1 = join_cli(31, files, tmp_path / "gaps1.ctx", gaps, extra=["--ncols", 1])
    g2 = join_cli(31, files, tmp_path / "gaps2.ctx", gaps, extra=["--ncols", 2])
    assert g1 == hdr + body and g2 == g1
    # to STDOUT, with the status lines
    rc, so, err = run(31, "join", "-o", "-", *gaps)
    assert rc == 0 and so == g1
    for line in ("Probing 3 graph files and 0 intersect files", "Output 5 cols; from 3 files; intersecting 0 graphs",
                 "[GReader] Loaded", "Dumped ", " kmers in 5 colours into: STDOUT"):
        assert line in err, (line, err)


def test_intersect_lines(mcx, tmp_path):
    files = build_samples(tmp_path, 31, 9)
    i0, i1, i2 = sorted(files)
    out = tmp_path / "isec.ctx"
    sizes = {p: len(files[p]) for p in (i1, i2)}
    assert sizes[i1] != sizes[i2]
    results = []
    for order in ([i1, i2], [i2, i1]):  # both command-line orders: the smaller one is swapped to the front
        got = join_cli(31, files, out, [i0, "1:" + i0], isec=order)
        hdr, body, st, _ = J.join_command([i0, "1:" + i0], files, order)
        assert got == hdr + body and st["kmers_written_no_covg"] > 0 and 0 < st["kmers_written"]
        results.append(got[len(hdr):])
        names = [g.cleaning.intersection_name for g in ctxio.read_header(got)[0]["ginfo"]]
        small, big = sorted(order, key=lambda p: sizes[p])
        first = "Sampe%d,Sampe%d" % (sorted(files).index(small), sorted(files).index(big))
        assert names == [first, first]
    assert results[0] == results[1]
    # one input without --sort: the k-mers nobody supplies are not written; with --sort they are
    for extra, keep in (([], False), (["--sort"], True)):
        got = join_cli(31, files, out, [i0], isec=[i1 + ":0"], extra=extra)
        hdr, body, st, _ = J.join_command([i0], files, [i1 + ":0"], sort=keep)
        assert got == hdr + body and (st["kmers_written_no_covg"] > 0) == keep


def test_intersect_graphs_of_equal_size(mcx, tmp_path):
    """two -i files with the same number of k-mers: no swap, so the mask comes from the first one given"""
    rng = random.Random(14)
    k = 31
    keys = pool(rng, k, 300)

    def write(name, sample, recs):
        g = ctxio.GraphInfo()
        g.sample_name = sample
        p = tmp_path / name
        p.write_bytes(ctxio.header_bytes(k, [g]) + J.pack(recs, k, 1))
        return str(p)

    # the same 200 keys in both, in another order and with other edges; a third of them with no coverage in `b`
    a = write("a.ctx", "Anna", [(key, [1], [rng.randrange(1, 256)]) for key in keys[:200]])
    b = write("b.ctx", "Bert", [(key, [i % 3], [rng.randrange(1, 256)]) for i, key in enumerate(reversed(keys[:200]))])
    inp = write("in.ctx", "In", [(key, [rng.randrange(1, 9)], [0xFF]) for key in keys[100:]])
    files = {p: open(p, "rb").read() for p in (a, b, inp)}
    assert len(files[a]) == len(files[b])
    out = tmp_path / "out.ctx"
    bodies = []
    for order, name in (([a, b], "Anna,Bert"), ([b, a], "Bert,Anna")):
        got = join_cli(31, files, out, ["0:" + inp, "0:" + inp], isec=order)
        hdr, body, st, _ = J.join_command(["0:" + inp, "0:" + inp], files, order)
        assert got == hdr + body
        assert 0 < st["kmers_written_no_covg"] < st["kmers_written"] == st["kmers_intersection"] < 200
        assert [g.cleaning.intersection_name for g in ctxio.read_header(got)[0]["ginfo"]] == [name]
        bodies.append(got[len(hdr):])
    assert len(bodies[0]) == len(bodies[1]) and bodies[0] != bodies[1]  # the same keys under another mask


@pytest.mark.parametrize("maxk,k", [(63, 33), (95, 67), (127, 99)])
def test_wider_binaries(mcx, tmp_path, maxk, k):
    files = build_samples(tmp_path, maxk, k, n=2)
    i0, i1 = sorted(files)
    args = ["1:" + i0, "0:" + i1, "1:" + i1]
    got = join_cli(maxk, files, tmp_path / "out.ctx", args)
    hdr, body, st, ncols = J.join_command(args, files)
    assert ncols == 2 and got == hdr + body and st["kmers_written"] > 100


def test_pipeline_after_join(mcx, tmp_path):
    files = build_samples(tmp_path, 31, 21)
    pop = tmp_path / "pop.ctx"
    rc, _, err = run(31, "join", "-q", "-o", pop, *sorted(files))
    assert rc == 0, err
    rc, _, err = run(31, "inferedges", "-q", "--pop", "-o", tmp_path / "pop.edges.ctx", pop)
    assert rc == 0, err
    rc, _, err = run(31, "popbubbles", "-q", "-o", tmp_path / "pop.popped.ctx", tmp_path / "pop.edges.ctx")
    assert rc == 0, err
    rc, so, err = run(31, "unitigs", "-q", tmp_path / "pop.popped.ctx")
    assert rc == 0 and so.startswith(b">unitig0 "), err
