"""tad_state_rollup's piecewise bucket function (theia_amd/csrc/tad_bucket.h: rollup_start) on the host: a stand-alone g++ program includes
the header alone — the function the roll-up's kernels call — floors the bound as tad_state_rollup does and prints rollup_start for the
quadruples on its standard input; Python's // is the reference.  Compiled plainly and with -fsanitize=address,undefined.  No GPU, no
library."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include "tad_bucket.h"
using namespace tad;

// stdin: lines "<t> <before_t> <bucket_s> <origin>"; stdout: "<bound> <image of t>" per line, then "lines <n>"
int main() {
  long long t, before, b, o;
  long lines = 0;
  while (scanf("%lld %lld %lld %lld", &t, &before, &b, &o) == 4) {
    if (!bucket_args_ok(b, o)) return 2;
    const int64_t bound = bucket_start(before, b, o);
    printf("%lld %lld\n", (long long)bound, (long long)rollup_start(t, bound, b, o));
    ++lines;
  }
  printf("lines %ld\n", lines);
  return 0;
}
"""


def floor_start(t, b, o):
    return o + b * ((t - o) // b)


def want(t, before, b, o):
    bound = floor_start(before, b, o)
    return bound, (floor_start(t, b, o) if t < bound else t)


def edge_table():
    out = []
    top = (1 << 62) - 1
    for b, o in ((1, 0), (60, 0), (60, 59), (60, 7), (3600, 1000), (86400, 0), ((1 << 32) + 1, 5), (1 << 40, (1 << 40) - 1)):
        for before in (0, 1, -1, o, o - 1, o + b, o - b, 1660202814, -1660202814, top, -top, 5 * b + o, 5 * b + o + b - 1, -5 * b + o):
            bound = floor_start(before, b, o)
            # at the bound, one below it, a bucket below it, the bound's own second bucket, the unfloored bound, below the origin, below zero
            for t in (bound, bound - 1, bound + 1, bound - b, bound - b - 1, bound + b - 1, before, before - 1, before + 1, o - 1, o, -1, 0, 1, -b,
                      top, -top):
                if abs(t) <= top:
                    out.append((t, before, b, o))
    return out


def seeded(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        b = int(rng.integers(1, (1 << 40) + 1)) if i % 3 == 0 else int(rng.integers(1, 100_000))
        o = int(rng.integers(0, b))
        before = int(rng.integers(-(1 << 62) + 1, 1 << 62)) if i % 2 == 0 else int(rng.integers(-5_000_000_000, 5_000_000_000))
        t = before + int(rng.integers(-3 * b, 3 * b + 1))
        if abs(t) < (1 << 62):
            out.append((t, before, b, o))
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_header_alone_against_the_floor(tmp_path, sanitize):
    src = tmp_path / "rollup_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "rollup_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "theia_amd", "csrc"), str(src), "-o", str(exe)])
    cases = edge_table() + seeded(20261021, 4000)
    lines = ["%d %d %d %d" % c for c in cases]
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.split("\n")
    assert got[len(lines)] == "lines %d" % len(lines)
    bad = [(c, got[i], want(*c)) for i, c in enumerate(cases) if got[i] != "%d %d" % want(*c)]
    assert not bad, bad[:10]


def test_the_table_holds_the_edges_and_the_images_keep_their_order():
    table = edge_table()
    at, below, moved, kept, under_origin, under_zero = (0,) * 6
    for t, before, b, o in table:
        bound, image = want(t, before, b, o)
        at += t == bound
        below += t == bound - 1 and image == bound - b
        moved += t < bound and image != t
        kept += t >= bound and image == t
        under_origin += t < o and t < bound and image <= t
        under_zero += t < 0 and t < bound
        assert (image < bound) == (t < bound) and image <= t                    # no bucket straddles the bound
    assert min(at, below, moved, kept, under_origin, under_zero) >= 8
    # strictly ascending times stay ascending (not strictly: equal images are what the roll-up folds), and every image below the bound
    # is a bucket start
    rng = np.random.default_rng(3)
    t = np.sort(rng.choice(np.arange(-5000, 5000), size=3000, replace=False))
    img = [want(int(x), 1234, 60, 7)[1] for x in t]
    bound = want(0, 1234, 60, 7)[0]
    assert bound == 1207 and all(a <= b for a, b in zip(img, img[1:]))
    assert all((x - 7) % 60 == 0 for x in img if x < bound) and [x for x in img if x >= bound] == [int(x) for x in t if x >= bound]
