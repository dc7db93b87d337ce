"""Times md5, sha1, sha224/256/384/512 and crc32 on the GPU over 4M rows of
32-byte strings and 4M rows of 200-byte strings (random lowercase letters),
and md5(concat_ws('|', a, b)) end to end over two 4M-row columns of 16-byte
strings. Each is the backend op on device columns: two warm-ups, then 9
runs, device events around the op. Next to each time stand the input bytes
per second it makes and the time it would take to only stream its bytes
(offsets and row bytes read, result and result offsets written) at the
6.3 TB/s that r02_roofline.md measured as achievable.

The CPU backend's hashlib / zlib path is timed on the first 1M of the same
rows (host clock, 3 runs) and scaled by 4, labelled as scaled.

Usage: python profiles/r18_digest_bench.py [out.json]
(results recorded in profiles/r18_digests.md)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spark_rapids_amd import Column, DType  # noqa: E402
from spark_rapids_amd.ops import cpu_backend as c  # noqa: E402
from spark_rapids_amd.ops import gpu_backend as g  # noqa: E402

STR = DType.string()
N, N_HOST, RUNS, HOST_RUNS = 4_000_000, 1_000_000, 9, 3
ROOF = 6.3e12  # bytes per second, profiles/r02_roofline.md
WIDTH = {"md5": 32, "sha1": 40, "sha224": 56, "sha256": 64, "sha384": 96,
         "sha512": 128}


def strings(n, width, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    data = torch.randint(97, 123, (n * width,), dtype=torch.uint8,
                         device="cuda", generator=gen)
    offs = torch.arange(0, (n + 1) * width, width, dtype=torch.int32,
                        device="cuda")
    return Column(STR, n, data, None, offs, 0)


def head(col, n):
    """The first n rows, on the host."""
    w = int(col.offsets[1])
    return Column(STR, n, col.data[:n * w].cpu(), None,
                  col.offsets[:n + 1].cpu(), 0)


def device_ms(fn):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    del out
    return start.elapsed_time(end)


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def gpu_case(res, name, fn, in_bytes, all_bytes):
    for _ in range(2):
        device_ms(fn)
    ms = [device_ms(fn) for _ in range(RUNS)]
    med = statistics.median(ms)
    res[name] = {"gpu_ms": ms, "gpu_median_ms": med, "input_bytes": in_bytes,
                 "input_gbytes_per_s": in_bytes / med / 1e6,
                 "streamed_bytes": all_bytes,
                 "stream_only_ms": all_bytes / ROOF * 1e3,
                 "times_stream_only": med / (all_bytes / ROOF * 1e3)}
    print(name, json.dumps(res[name]), flush=True)
    torch.cuda.empty_cache()


def host_case(res, name, fn):
    ms = [host_ms(fn) for _ in range(HOST_RUNS)]
    med = statistics.median(ms)
    scaled = med * N / N_HOST
    res[name].update(host_1m_ms=ms, host_1m_median_ms=med,
                     host_scaled_to_4m_ms=scaled,
                     cpu_over_gpu=scaled / res[name]["gpu_median_ms"])
    print(name, "host", json.dumps(ms), flush=True)


def main():
    res = {"rows": N, "host_rows": N_HOST, "runs": RUNS,
           "device": torch.cuda.get_device_name(0)}
    for width in (32, 200):
        col = strings(N, width, width)
        hcol = head(col, N_HOST)
        in_bytes = N * width
        read = in_bytes + 4 * (N + 1)
        for algo, w in WIDTH.items():
            name = f"{algo}_{width}B"
            gpu_case(res, name, lambda: g.digest_hex(col, algo), in_bytes,
                     read + N * w + 4 * (N + 1))
            host_case(res, name, lambda: c.digest_hex(hcol, algo))
        name = f"crc32_{width}B"
        gpu_case(res, name, lambda: g.crc32(col), in_bytes, read + 8 * N)
        host_case(res, name, lambda: c.crc32(hcol))
        del col
        torch.cuda.empty_cache()
    a, b = strings(N, 16, 1), strings(N, 16, 2)
    ha, hb = head(a, N_HOST), head(b, N_HOST)
    in_bytes = 2 * N * 16
    joined = in_bytes + N
    gpu_case(res, "md5_concat_ws", lambda: g.digest_hex(
        g.concat_ws("|", [a, b]), "md5"), in_bytes,
        in_bytes + 2 * 4 * (N + 1) + 2 * (joined + 4 * (N + 1)) +
        32 * N + 4 * (N + 1))
    host_case(res, "md5_concat_ws", lambda: c.digest_hex(
        c.concat_ws("|", [ha, hb]), "md5"))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
