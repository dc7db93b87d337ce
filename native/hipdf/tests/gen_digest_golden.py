"""Write tests/golden/digest_expected.txt: what hashlib and zlib give for the
messages digest_host_test.cpp builds. One line per algorithm and message
length 0..260: `<algorithm> <length> <lowercase hex>`; byte i of the message
of length n is (7 * i + 131 * n) & 0xFF. crc32 is printed as 8 hex digits.

Run from the repository root: python native/hipdf/tests/gen_digest_golden.py
"""
import hashlib
import os
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))))
ALGOS = ("md5", "sha1", "sha224", "sha256", "sha384", "sha512")
MAX_LEN = 260


def message(n: int) -> bytes:
    return bytes((7 * i + 131 * n) & 0xFF for i in range(n))


def lines():
    for algo in ALGOS:
        for n in range(MAX_LEN + 1):
            yield f"{algo} {n} {hashlib.new(algo, message(n)).hexdigest()}"
    for n in range(MAX_LEN + 1):
        yield f"crc32 {n} {zlib.crc32(message(n)) & 0xFFFFFFFF:08x}"


def main():
    out = os.path.join(REPO, "tests", "golden", "digest_expected.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines()) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
