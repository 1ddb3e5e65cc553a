"""The byte-level LIKE matcher in plain Python: what tad_strdict_like (include/tad.h, theia_amd/csrc/tad_like.h) must compute, bit for
bit.  It never calls the engine.  The rules are those of theia_amd.anomaly_detection._like_regex, on bytes:
  \\ + byte -> that byte as a literal (a trailing lone \\ is a literal backslash); % -> any run of bytes, the empty one included;
  _ -> one character; anything else a literal; the pattern matches the whole value; with nocase 'A'..'Z' fold to 'a'..'z', nothing else.
One character = the byte at the position, whatever it is, then every following byte in 0x80..0xBF — one code point on well-formed
UTF-8, and THE definition on malformed bytes.  The position a % retries from advances by the same step."""

LIT, ONE, ANY = 0, 1, 2


def fold(c):
    return c + 32 if 0x41 <= c <= 0x5A else c


def compile_like(pattern, nocase=False):
    """pattern bytes -> (tokens, min_len): tokens are (LIT, byte), (ONE, None), (ANY, None); min_len = the least bytes a match needs"""
    pattern = bytes(pattern)
    toks, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if c == 0x5C and i + 1 < len(pattern):
            i += 1
            toks.append((LIT, fold(pattern[i]) if nocase else pattern[i]))
        elif c == 0x25:
            if not toks or toks[-1][0] != ANY:
                toks.append((ANY, None))
        elif c == 0x5F:
            toks.append((ONE, None))
        else:
            toks.append((LIT, fold(c) if nocase else c))
        i += 1
    return toks, sum(1 for k, _ in toks if k != ANY)


def char_end(value, i):
    """the position behind the character that starts at i"""
    i += 1
    while i < len(value) and 0x80 <= value[i] <= 0xBF:
        i += 1
    return i


FOLD = bytes(fold(c) for c in range(256))


def segments(toks):
    """the tokens split at every %: [tokens in front of the first %, between the first and the second, ..., behind the last]"""
    segs, cur = [], []
    for t in toks:
        if t[0] == ANY:
            segs.append(cur)
            cur = []
        else:
            cur.append(t)
    segs.append(cur)
    return segs


def fits(seg, value, at, to_end):
    """the %-free tokens seg at value[at:]: the position behind them, or -1; to_end: they must reach the value's end"""
    n = len(value)
    for kind, c in seg:
        if at >= n:
            return -1
        if kind == ONE:
            at = char_end(value, at)
        elif value[at] == c:
            at += 1
        else:
            return -1
    return at if not to_end or at == n else -1


def match_segments(segs, value, nocase=False):
    """the segments against the WHOLE value.  A pattern without % is walked once; a % tries what stands behind it at every character
    start from where it was met, left to right, and the first place where the tokens up to the next % (or the end) fit is kept —
    which decides the same as trying every place."""
    if nocase:
        value = value.translate(FOLD)
    n = len(value)
    if len(segs) == 1:
        return fits(segs[0], value, 0, True) == n
    at = fits(segs[0], value, 0, False)               # in front of the first %: anchored at the start
    if at < 0:
        return False
    for k in range(1, len(segs)):
        seg, last = segs[k], k == len(segs) - 1
        if last and not seg:                          # a trailing % takes the rest
            return True
        start = at
        while True:
            end = fits(seg, value, start, last)
            if end >= 0:
                break
            if start >= n:
                return False
            start = char_end(value, start)
        at = end
    return True


def match_tokens(toks, value, nocase=False):
    return match_segments(segments(toks), bytes(value), nocase)


def like_match(pattern, value, nocase=False):
    toks, need = compile_like(pattern, nocase)
    if len(value) < need:
        return False
    return match_tokens(toks, value, nocase)


def like_mask(pattern, values, nocase=False):
    """[0 / 1 per value] for a list of bytes"""
    toks, need = compile_like(pattern, nocase)
    segs = segments(toks)
    return [1 if len(v) >= need and match_segments(segs, v, nocase) else 0 for v in values]


# ---- the cases the host test and the GPU test share ----
# (pattern, value, nocase match, case-sensitive match)
TABLE = [
    ("", "", True, True), ("", "a", False, False),
    ("%", "", True, True), ("%", "anything\nat all", True, True),
    ("_", "", False, False), ("_", "a", True, True), ("_", "é", True, True), ("_", "日", True, True), ("_", "ab", False, False), ("_", "\n", True, True),
    ("__", "a", False, False), ("__", "é", False, False), ("__", "é日", True, True), ("__", "abc", False, False),
    ("%_", "", False, False), ("%_", "x", True, True), ("_%", "", False, False), ("_%", "日本", True, True),
    ("a%", "abc", True, True), ("a%", "Abc", True, False), ("a%", "ba", False, False), ("a%", "a", True, True),
    ("%a", "bca", True, True), ("%a", "bcA", True, False), ("%a", "ab", False, False),
    ("a%b%c", "abc", True, True), ("a%b%c", "aXXbYYc", True, True), ("a%b%c", "acb", False, False), ("a%b%c", "abcb", False, False), ("a%b%c", "aBbC", True, False),
    ("%a_c%", "abc", True, True), ("%a_c%", "xxa日cyy", True, True), ("%a_c%", "ac", False, False), ("%a_c%", "xA\ncx", True, False), ("%a_c%", "abbc", False, False),
    ("\\%", "%", True, True), ("\\%", "a", False, False), ("\\%", "", False, False),
    ("\\_", "_", True, True), ("\\_", "a", False, False),
    ("\\\\", "\\", True, True), ("\\\\", "\\\\", False, False),
    ("a\\", "a\\", True, True), ("a\\", "a", False, False), ("\\", "\\", True, True),
    ("%ab\\%", "xxab%", True, True), ("%ab\\%", "xxab%y", False, False), ("%ab\\%", "xxab", False, False), ("%ab\\%", "AB%", True, False),
    ("%%", "", True, True), ("%%", "abc", True, True), ("a%%b", "ab", True, True), ("a%%b", "a12b", True, True),
    ("%a%a%a%b", "a" * 64, False, False), ("%a%a%a%b", "a" * 63 + "b", True, True), ("%a%a%a%b", "aab", False, False), ("%a%a%a%b", "aaab", True, True),
    ("%\"test_key\":\"test_value\"%", "{\"app\":\"db\",\"test_key\":\"test_value\"}", True, True),
    ("%\"test_key\":\"test_value\"%", "{\"testXkey\":\"TEST-value\"}", True, False),
    ("%test\\_key%", "{\"testXkey\":\"v\"}", False, False), ("%test\\_key%", "{\"TEST_key\":\"v\"}", True, False),
    ("\\A", "a", True, False), ("\\a", "A", True, False),
]

MALFORMED = [b"\x80", b"\x80\x80a", b"\xbfa", b"a\xc3", b"\xe6\x97", b"\xe6\x97\xa5\xe6", b"\xc3\xc3\xa9", b"a\x80\x80\x80b", b"\xff\xfe", b"\x80a\xc3", b"\xa9\xc3\xa9\xc3",
             b"\xe6a\x97\xa5"]
MALFORMED_PATTERNS = [b"_", b"__", b"___", b"%_", b"_%", b"%_a", b"a_", b"_a%", b"%a_", b"%_\xc3", b"\xc3_", b"%\x80%", b"_\xa9", b"%__%", b"a%_b", b"%\xe6_", b"_\x97\xa5", b"%"]
