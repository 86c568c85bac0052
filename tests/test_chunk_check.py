"""The host read chunker (mccortex_amd/csrc/mcx_chunk.h) on the CPU: chunk_check.cpp is built with the host compiler
under the address and undefined-behaviour sanitizers and run as a child process.  It fills buffers of exactly the size
each staging layout allows, at the sizes where the filler changes branch, and exits non-zero on any violation."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mccortex_amd", "csrc")


def test_chunker_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chunk_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + CSRC, os.path.join(HERE, "chunk_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    assert p.stdout.decode().strip() == "chunk_check: ok"
