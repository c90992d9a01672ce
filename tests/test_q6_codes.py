"""The host translation of Q6's predicate bounds into the code domain of a
column image (monetdb_amd/csrc/q6codes.h), compiled alone into
tests/q6codes_check.cpp's program and run on the CPU -- under
-fsanitize=undefined where the compiler links it, since signed overflow is
what goes wrong in such arithmetic."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_code_bounds_match_raw_predicate(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(HERE, "q6codes_check.cpp")
    exe = str(tmp_path / "q6codes_check")
    base = [cxx, "-std=c++17", "-O1", "-Wall", src, "-o", exe]
    san = ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)   # no sanitizer runtime here
        assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith(" 0 wrong")
