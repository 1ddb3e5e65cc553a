"""The bucket arithmetic (theia_amd/csrc/tad_bucket.h) on the host: a stand-alone g++ program includes the header alone — the very
function the kernels of tad_window.hip and the checks of tad_capi_view.cpp call — and prints bucket_start for the triples on its standard
input; Python's // (the mathematical floor on integers of any size) is the reference.  Compiled plainly and with
-fsanitize=address,undefined: inside AND outside the documented domain nothing may overflow a signed integer.  No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

import buckets_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include "tad_bucket.h"
using namespace tad;

// stdin: lines "<t> <bucket_s> <origin>"; stdout: "<ok> <start>" per line, then "lines <n>"
int main() {
  long long t, b, o;
  long lines = 0;
  while (scanf("%lld %lld %lld", &t, &b, &o) == 3) {
    const bool ok = bucket_args_ok(b, o);
    printf("%d %lld\n", ok ? 1 : 0, ok ? (long long)bucket_start(t, b, o) : 0ll);
    ++lines;
  }
  printf("lines %ld\n", lines);
  return kBucketMaxSeconds == ((int64_t)1 << 40) ? 0 : 1;
}
"""


def floor_start(t, b, o):
    return o + b * ((t - o) // b)


def edge_table():
    out = []
    top = (1 << 62) - 1
    for b in (1, 2, 60, 3600, 86400, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 40):
        for o in sorted({0, 1, b // 2, b - 1}):
            if not 0 <= o < b:
                continue
            for t in (-1, 0, 1, b - 1, b, b + 1, -b, -b - 1, -b + 1, o - 1, o, o + 1, o - b, o + b, top, -top, top - b, -top + b,
                      (1 << 32) - 1, 1 << 32, -(1 << 32), 1660202814, -1660202814):
                out.append((t, b, o))
    return out


def seeded_triples(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        b = int(rng.integers(1, (1 << 40) + 1)) if i % 3 == 0 else int(rng.integers(1, 100_000))
        o = int(rng.integers(0, b))
        t = int(rng.integers(-(1 << 62) + 1, 1 << 62)) if i % 2 == 0 else int(rng.integers(-5_000_000_000, 5_000_000_000))
        out.append((t, b, o))
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_header_alone_against_the_floor(tmp_path, sanitize):
    src = tmp_path / "bucket_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "bucket_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "theia_amd", "csrc"), str(src), "-o", str(exe)])
    cases = edge_table() + seeded_triples(20250917, 4000)
    refused = [(5, 0, 0), (5, -60, 0), (5, 60, -1), (5, 60, 60), (5, 1, 1)]
    # outside the domain: defined (no sanitizer report); the start wraps and is held to nothing
    outside = [((1 << 63) - 1, 60, 0), (-(1 << 63), 60, 59), (-(1 << 63), (1 << 62) + 5, 7), ((1 << 63) - 1, (1 << 63) - 1, (1 << 63) - 2)]
    lines = ["%d %d %d" % c for c in cases + refused + outside]
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.split("\n")
    assert got[len(lines)] == "lines %d" % len(lines)
    bad = [(c, got[i]) for i, c in enumerate(cases) if got[i] != "1 %d" % floor_start(*c)]
    assert not bad, bad[:10]
    assert all(got[len(cases) + i] == "0 0" for i in range(len(refused)))
    for i in range(len(outside)):                                        # (some start, whatever the wrap gives; the sanitizer saw no overflow)
        assert got[len(cases) + len(refused) + i].startswith("1 "), (outside[i], got[len(cases) + len(refused) + i])
    # the numpy model computes the same starts wherever int64 holds the intermediate
    small = [(t, b, o) for t, b, o in cases if abs(t) < (1 << 61)]
    for t, b, o in small[::7]:
        assert int(M.bucket_start(np.array([t]), b, o)[0]) == floor_start(t, b, o), (t, b, o)


def test_the_table_holds_every_edge_the_contract_names():
    table = edge_table()
    for b in (1, 1 << 40):
        assert any(c[1] == b for c in table)
    for t, b, o in ((-1, 60, 0), (0, 60, 0), (59, 60, 0), (60, 60, 0), (58, 60, 59), (59, 60, 59), ((1 << 62) - 1, 60, 0), (-(1 << 62) + 1, 60, 0)):
        assert (t, b, o) in table, (t, b, o)
    assert floor_start(-1, 60, 0) == -60 and floor_start(58, 60, 59) == -1 and floor_start(-1, 60, 59) == -1
