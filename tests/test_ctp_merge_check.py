"""The header merger of `pjoin` (mccortex_amd/host/ctp_merge.c) on the CPU: ctp_merge_check.c is built with the host
compiler under the address and undefined-behaviour sanitizers and run as a child process.  Quotes and braces inside sample
names, an empty commands array, a command key that two inputs share, a colour no input fills, a histogram with no entries,
lists of two lengths, two names for one colour; it exits non-zero on any violation."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "mccortex_amd", "host")


def test_ctp_merge_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ctp_merge_check")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-DMAX_KMER_SIZE=31", "-I" + HOST, os.path.join(HERE, "ctp_merge_check.c"), os.path.join(HOST, "ctp_merge.c"),
                           os.path.join(HOST, "ctp_hdr.c"), os.path.join(HOST, "host_util.c"), "-o", exe, "-lz", "-lm"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    assert p.stdout.decode().strip() == "ctp_merge_check: ok"
