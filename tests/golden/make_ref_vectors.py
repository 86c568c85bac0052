#!/usr/bin/env python3
"""Regenerates tests/golden/reference_vectors.npz from the reference code compiled into oracle/_ref
(run from the repo root after build(), on a machine where the reference tree was present at build time).

The tests in tests/test_oracle.py and tests/test_host_sizing.py compare the oracle and the product against
the reference's own lookup3.h, kmer_hash.h, revcmp.c and hash_mem.h.  oracle/_ref exists only where the
reference could be compiled; this file freezes what those libraries answered for the tests' fixed inputs,
so that the same comparisons run everywhere (and, where oracle/_ref exists, the tests check the stored
answers against it as well).

Arrays (all uint64):
  lk3_k<k>      [n, W + 2]   k-mer words (word 0 on the left), initval, ref_lk3_hashlittle(words, 8 W, initval)
  bklk3_k<k>    [n, W + 2]   canonical key words, initval, ref_bklk3_hashlittle(key, initval)
  revcmp_k<k>   [n, 2 W]     k-mer words, reverse-complement words (all four revcmp methods agree)
  hashmem_const [4]          REHASH_LIMIT, MAX_BUCKET_SIZE, bits of (float) IDEAL_OCCUPANCY, WARN_OCCUPANCY
  hashmem_kmers [n, 5]       nkmers, bits per entry, bucket_size, nbuckets, ht_mem  (plans for a k-mer count)
  hashmem_mem   [n, 5]       memory, bits per entry, bucket_size, nbuckets, ht_mem  (plans for a memory limit)
"""
import ctypes as C
import os
import random
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_vectors.npz")

LK3_KS = (3, 15, 31, 33, 47, 63, 65, 95, 127)
BKLK3_KS = (3, 15, 29, 31, 33, 47, 63, 65, 79, 95, 97, 111, 127)
REVCMP_KS = tuple(range(3, 128, 2))
HASHMEM_BITS = (104, 168, 288)
HASHMEM_MEMS = (1 << 20, 512 << 20, 70 << 30)


def rand_kmer(rng, k):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, k))


def words(x, W):
    return [int(x.b[i]) for i in range(W)]


def lk3(L, R):
    out = {}
    rng = np.random.default_rng(1)
    for k in LK3_KS:
        W = L.orc_words_for_k(k)
        rows = []
        for _ in range(200):
            x = L.orc_kmer_from_str(rand_kmer(rng, k).encode(), k)
            iv = int(rng.integers(0, 2**32))
            a = np.array(words(x, W), dtype=np.uint64)
            rows.append(words(x, W) + [iv, R.ref_lk3_hashlittle(a.ctypes.data, 8 * W, iv)])
        out["lk3_k%d" % k] = np.array(rows, dtype=np.uint64)
    return out


def bklk3(L):
    out = {}
    for k in BKLK3_KS:
        W = L.orc_words_for_k(k)
        R = orc.ref_revcmp(W)
        rng = np.random.default_rng(500 + k)
        rows = []
        for s in [rand_kmer(rng, k) for _ in range(300)] + ["A" * k, "T" * k, "ACG" * (k // 3) + "A" * (k % 3)]:
            key = words(L.orc_kmer_get_key(L.orc_kmer_from_str(s.encode(), k), k), W)
            a = np.array(key, dtype=np.uint64)
            for iv in (0, 1, 7, int(rng.integers(0, 2**32))):
                rows.append(key + [iv, R.ref_bklk3_hashlittle(a.ctypes.data, iv)])
        out["bklk3_k%d" % k] = np.array(rows, dtype=np.uint64)
    return out


def revcmp(L):
    out = {}
    for k in REVCMP_KS:
        W = L.orc_words_for_k(k)
        R = orc.ref_revcmp(W)
        rng = np.random.default_rng(100 + k)
        rows = []
        for s in [rand_kmer(rng, k) for _ in range(60)] + ["A" * k, "T" * k, "C" * k, "G" * k, "AC" * (k // 2) + "G"]:
            fw = words(L.orc_kmer_from_str(s.encode(), k), W)
            a = np.array(fw, dtype=np.uint64)
            want = None
            for method in (1, 2, 3, 4):
                o = np.zeros(W, dtype=np.uint64)
                R.ref_revcmp(method, a.ctypes.data, k, o.ctypes.data)
                got = [int(w) for w in o]
                assert want is None or got == want, (k, s, method)
                want = got
            rows.append(fw + want)
        out["revcmp_k%d" % k] = np.array(rows, dtype=np.uint64)
    return out


def hashmem(R):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_sizing import Plan
    H = C.CDLL(os.path.join(ROOT, "mccortex_amd", "bin", "libmcxhost.so"))
    H.table_plan_for_kmers.restype = Plan
    H.table_plan_for_kmers.argtypes = [C.c_uint64, C.c_size_t]
    H.table_plan_for_memory.restype = Plan
    H.table_plan_for_memory.argtypes = [C.c_size_t, C.c_size_t]
    f32 = lambda v: struct.unpack("<I", struct.pack("<f", v))[0]
    const = [R.ref_rehash_limit(), R.ref_max_bucket_size(), f32(R.ref_ideal_occupancy()), f32(R.ref_warn_occupancy())]
    kmers, mems = [], []
    rnd = random.Random(3)
    for bits in HASHMEM_BITS:
        for _ in range(200):
            nk = rnd.randrange(1, 1 << rnd.randrange(4, 40))
            p = H.table_plan_for_kmers(nk, bits)
            kmers.append([nk, bits, p.bucket_size, p.nbuckets, R.ref_ht_mem(p.bucket_size, p.nbuckets, bits)])
        for mem in HASHMEM_MEMS:
            p = H.table_plan_for_memory(mem, bits)
            mems.append([mem, bits, p.bucket_size, p.nbuckets, R.ref_ht_mem(p.bucket_size, p.nbuckets, bits)])
    return {"hashmem_const": np.array(const, dtype=np.uint64), "hashmem_kmers": np.array(kmers, dtype=np.uint64),
            "hashmem_mem": np.array(mems, dtype=np.uint64)}


if __name__ == "__main__":
    L = orc.lib()
    R3, RH = orc.ref_lookup3(), orc.ref_hashmem()
    if R3 is None or RH is None or any(orc.ref_revcmp(W) is None for W in (1, 2, 3, 4)) or \
            not hasattr(orc.ref_revcmp(1), "ref_bklk3_hashlittle"):
        raise SystemExit("oracle/_ref is incomplete: run build() where the reference tree is present")
    arrays = {}
    arrays.update(lk3(L, R3))
    arrays.update(bklk3(L))
    arrays.update(revcmp(L))
    arrays.update(hashmem(RH))
    np.savez_compressed(OUT, **arrays)
    print("%s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))
