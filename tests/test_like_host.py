"""The LIKE pattern language (theia_amd/csrc/tad_like.h) on the host.  Two steps: the plain-Python byte-level matcher of tests/like_ref.py is
held against the regex the batch job builds (theia_amd.anomaly_detection._like_regex) on well-formed UTF-8 — a hand-written table and a few
thousand seeded pairs —, and a stand-alone g++ program that includes tad_like.h alone (like_compile and like_match, the code k_sd_like
runs) is held against that reference on the same pairs plus malformed values, with and without TAD_LIKE_NOCASE.  No GPU, no library.
Kept out of every value: U+212A, U+017F, U+0130 and U+0131 (re.IGNORECASE lets k, s and i match them) and capitals outside ASCII (no
Unicode case folding on bytes), and a newline as a value's last byte (re's $ matches in front of it; a test below pins that)."""
import os
import re
import subprocess

import numpy as np
import pytest

import like_ref
from theia_amd.anomaly_detection import _like_regex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE, MALFORMED, MALFORMED_PATTERNS = like_ref.TABLE, like_ref.MALFORMED, like_ref.MALFORMED_PATTERNS

ALPHABETS = ("ab%_", "aAbB%_\\", "ab%_\\'\"éx", "aé日%_", "abc_%XY\n")


def regex_says(pattern, value, nocase):
    rx = _like_regex(pattern)
    if not nocase:
        rx = re.compile(rx.pattern, re.DOTALL)        # the same translation, without the case fold
    return rx.match(value) is not None


def seeded_pairs(seed, n):
    """(pattern, value) strings over small alphabets — collisions are what makes a wildcard matter — a third of the patterns in the
    '%' + text + '%' form the job builds.  Values draw from the WHOLE alphabet, %, _ and \\ included, so that an escaped literal in
    the pattern can meet its byte in the value"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        alpha = ALPHABETS[i % len(ALPHABETS)]
        p = "".join(alpha[j] for j in rng.integers(0, len(alpha), int(rng.integers(0, 7))))
        if i % 3 == 0:
            p = "%" + p + "%"
        v = "".join(alpha[j] for j in rng.integers(0, len(alpha), int(rng.integers(0, 9))))
        if i % 4 == 0 and alpha != ALPHABETS[0]:
            v = v.upper() if "é" not in alpha else v.replace("a", "A").replace("x", "X")
        if v.endswith("\n"):                           # re's $ also matches in front of a trailing newline: see test_a_trailing_newline_...
            v += "a"
        out.append((p, v))
    return out


PAIRS = seeded_pairs(20240611, 4000)


def test_the_table_says_what_the_regex_says():
    for p, v, want_nocase, want_case in TABLE:
        assert regex_says(p, v, True) == want_nocase, (p, v)
        assert regex_says(p, v, False) == want_case, (p, v)


def test_a_trailing_newline_is_the_one_place_where_the_regex_is_not_anchored():
    """Python's $ matches at the end AND in front of a newline that ends the value, so the regex of a pattern that does not end in %
    accepts one trailing newline that LIKE — and the reference — do not.  The job's '%label%' form ends in % and is not touched."""
    assert regex_says("a", "a\n", True) and not like_ref.like_match(b"a", b"a\n", True)
    assert regex_says("", "\n", False) and not like_ref.like_match(b"", b"\n", False)
    assert not regex_says("a", "a\n\n", True) and not regex_says("a", "\na", True)
    for p in ("%a%", "a%", "%"):
        assert regex_says(p, "a\n", True) and like_ref.like_match(p.encode(), b"a\n", True)


def test_reference_agrees_with_the_table():
    for p, v, want_nocase, want_case in TABLE:
        assert like_ref.like_match(p.encode(), v.encode(), True) == want_nocase, (p, v)
        assert like_ref.like_match(p.encode(), v.encode(), False) == want_case, (p, v)


def test_reference_agrees_with_the_regex_on_seeded_pairs():
    hits = escaped_hits = 0
    for p, v in PAIRS:
        for nocase in (True, False):
            want = regex_says(p, v, nocase)
            assert like_ref.like_match(p.encode(), v.encode(), nocase) == want, (p, v, nocase)
            hits += want
            escaped_hits += want and "\\" in p.strip("%")
    assert 0.1 * len(PAIRS) < hits < 1.9 * len(PAIRS)       # both answers are well represented
    assert escaped_hits >= 10                               # and so is a match through an escaped literal (\%, \_, \\)


def test_compile_step_of_the_reference():
    L, O, A = like_ref.LIT, like_ref.ONE, like_ref.ANY
    assert like_ref.compile_like(b"") == ([], 0)
    assert like_ref.compile_like(b"%%%") == ([(A, None)], 0)
    assert like_ref.compile_like(b"a%%_%b") == ([(L, 97), (A, None), (O, None), (A, None), (L, 98)], 3)
    assert like_ref.compile_like(b"\\%\\_\\\\\\") == ([(L, 0x25), (L, 0x5F), (L, 0x5C), (L, 0x5C)], 4)
    assert like_ref.compile_like(b"%ab\\%") == ([(A, None), (L, 97), (L, 98), (L, 0x25)], 3)
    assert like_ref.compile_like(b"A\\Z[\xc9", True) == ([(L, 97), (L, 122), (L, 0x5B), (L, 0xC9)], 4)     # 'A'..'Z' and nothing else
    assert like_ref.compile_like(b"A\\Z", False) == ([(L, 65), (L, 90)], 2)


def test_malformed_values_by_the_character_rule():
    """one character = a byte and the continuation bytes behind it, wherever it stands"""
    m = like_ref.like_match
    assert m(b"_", b"\x80") and m(b"_", b"\x80\x80\x80") and not m(b"__", b"\x80\x80\x80")       # a leading run of continuation bytes is one character
    assert m(b"_a", b"\x80\x80a") and m(b"__", b"a\xc3") and m(b"a_", b"a\xc3")                    # a lead byte cut off at the end is one
    assert m(b"__", b"\xc3\xc3\xa9") and not m(b"_", b"\xc3\xc3\xa9")
    assert m(b"_", b"\xe6\x97") and m(b"__", b"\xe6\x97\xa5\xe6") and m(b"__", b"\xff\xfe")
    assert m(b"%_\xc3", b"\x80a\xc3") and not m(b"%_\xa9", b"\xc3\xa9")                            # the retry never lands inside a character
    assert m(b"a_b", b"a\x80\x80\x80b") and m(b"a__", b"a\x80\x80\x80b") and not m(b"a____", b"a\x80\x80\x80b")


PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tad_like.h"
using namespace tad;

// stdin: lines "<flags> <pattern hex or -> <value hex or ->"; stdout: one 0 / 1 per line, then "min <least length>" per line
static std::vector<uint8_t> unhex(const char *s) {
  std::vector<uint8_t> out;
  if (s[0] == '-') return out;
  for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
    unsigned x = 0;
    sscanf(s + i, "%2x", &x);
    out.push_back((uint8_t)x);
  }
  return out;
}

int main() {
  static char p[8192], v[8192];
  unsigned flags = 0;
  static uint16_t tok[kLikeMaxTokens];
  long lines = 0;
  while (scanf("%u %8191s %8191s", &flags, p, v) == 3) {
    const std::vector<uint8_t> pat = unhex(p), val = unhex(v);
    if (pat.size() > kLikeMaxTokens) { printf("pattern too long\n"); return 1; }
    uint32_t min_len = ~0u;
    const uint32_t n = like_compile(pat.data(), (uint32_t)pat.size(), flags, tok, &min_len);
    if (n > pat.size() || min_len > n) { printf("program of %u tokens, least length %u from %zu bytes\n", n, min_len, pat.size()); return 1; }
    long asked = 0;
    const uint32_t len = (uint32_t)val.size();
    auto byte = [&](uint32_t i) -> uint32_t {
      if (i >= len) { printf("byte %u of %u asked\n", i, len); exit(1); }
      ++asked;
      return val[i];
    };
    const bool hit = len >= min_len && like_match([&](uint32_t k) -> uint32_t { return tok[k]; }, n, byte, len, (flags & kLikeNocase) != 0);
    if (asked > 2l * ((long)len + 1) * ((long)n + 1)) { printf("%ld bytes asked for %u bytes x %u tokens\n", asked, len, n); return 1; }
    printf("%d %u\n", hit ? 1 : 0, min_len);
    ++lines;
  }
  printf("lines %ld\n", lines);
  return 0;
}
"""


def _hex(b):
    return b.hex() if b else "-"


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_header_alone_against_the_reference(tmp_path, sanitize):
    src = tmp_path / "like_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "like_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "theia_amd", "csrc"), str(src), "-o", str(exe)])
    cases = [(p.encode(), v.encode()) for p, v, _, _ in TABLE] + [(p.encode(), v.encode()) for p, v in PAIRS]
    cases += [(p, v) for p in MALFORMED_PATTERNS for v in MALFORMED]
    cases += [(b"%" + b"a_" * 511 + b"%", b"ab" * 300), (b"_" * 1024, b"x" * 1024), (b"_" * 1024, b"x" * 1023), (b"\\" * 1024, b"\\" * 512), (b"%" * 1024, b"")]
    lines, want = [], []
    for p, v in cases:
        for f in (0, 1):
            lines.append("%d %s %s" % (f, _hex(p), _hex(v)))
            want.append("%d %d" % (like_ref.like_match(p, v, bool(f)), like_ref.compile_like(p, bool(f))[1]))
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.split("\n")
    assert got[len(lines)] == "lines %d" % len(lines)
    bad = [(lines[i], got[i], want[i]) for i in range(len(lines)) if got[i] != want[i]]
    assert not bad, bad[:10]
