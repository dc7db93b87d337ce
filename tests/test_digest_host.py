"""The digest cores (native/hipdf/kernels/digest.h: MD5, SHA-1, SHA-2, CRC-32,
the row reader and the hex writer) run on the host under the sanitizers as a
stand-alone program, against what hashlib and zlib give
(tests/golden/digest_expected.txt, written by
native/hipdf/tests/gen_digest_golden.py)."""
import hashlib
import os
import shutil
import subprocess
import zlib

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "native", "hipdf")
GOLDEN = os.path.join(REPO, "tests", "golden", "digest_expected.txt")
ALGOS = ("md5", "sha1", "sha224", "sha256", "sha384", "sha512")


@pytest.fixture(scope="module")
def digest_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("dg") / "digest_host_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall",
                    "-fsanitize=address,undefined",
                    "-I" + os.path.join(NATIVE, "kernels"),
                    os.path.join(NATIVE, "tests", "digest_host_test.cpp"),
                    "-o", exe], check=True)
    return exe


def _message(n: int) -> bytes:
    return bytes((7 * i + 131 * n) & 0xFF for i in range(n))


def test_golden_file_is_what_hashlib_gives():
    """The committed fixture is the generator's output, line for line."""
    want = [f"{a} {n} {hashlib.new(a, _message(n)).hexdigest()}"
            for a in ALGOS for n in range(261)]
    want += [f"crc32 {n} {zlib.crc32(_message(n)) & 0xFFFFFFFF:08x}"
             for n in range(261)]
    with open(GOLDEN) as f:
        assert f.read().splitlines() == want


def test_known_answers_and_every_length(digest_exe):
    run = subprocess.run([digest_exe, GOLDEN], capture_output=True, text=True)
    print(run.stdout[-3000:])
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-4000:])
    assert f"cases {7 * 261} alignments 16 failures 0" in run.stdout


def test_a_wrong_expectation_fails(digest_exe, tmp_path):
    """The program does compare: one flipped digit is a failure."""
    with open(GOLDEN) as f:
        lines = f.read().splitlines()
    algo, n, hexd = lines[70].split()
    lines[70] = f"{algo} {n} {'1' if hexd[0] == '0' else '0'}{hexd[1:]}"
    bad = tmp_path / "bad.txt"
    bad.write_text("\n".join(lines[:200]) + "\n")
    run = subprocess.run([digest_exe, str(bad)], capture_output=True,
                         text=True)
    assert run.returncode == 1 and f"FAIL {algo} len {n} " in run.stdout
