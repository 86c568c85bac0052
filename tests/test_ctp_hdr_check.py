"""The .ctp header reader / editor and the piece cutter of `links` (mccortex_amd/host/ctp_hdr.c) on the CPU:
ctp_hdr_check.c is built with the host compiler under the address and undefined-behaviour sanitizers and run as a child
process.  Braces and quotes inside strings, an empty commands array, numbers at the end of an object, a header cut short
at every length, a block larger than the buffer, a piece that ends inside a k-mer line, a file without a trailing
newline; it exits non-zero on any violation."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "mccortex_amd", "host")


def test_ctp_header_and_pieces_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ctp_hdr_check")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-DMAX_KMER_SIZE=31", "-I" + HOST, os.path.join(HERE, "ctp_hdr_check.c"), os.path.join(HOST, "ctp_hdr.c"),
                           os.path.join(HOST, "host_util.c"), "-o", exe, "-lz", "-lm"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    assert p.stdout.decode().strip() == "ctp_hdr_check: ok"
