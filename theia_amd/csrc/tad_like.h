// tad_like.h — the LIKE / ilike pattern language of tad_strdict_like (tad.h): the compile step (pattern bytes -> a token program, on the
// host) and the matcher (a token program against one value's bytes, on the host and in k_sd_like).  The one place that says what %, _
// and \ mean.  The parity contract is theia_amd/anomaly_detection.py:_like_regex — the regex the batch job builds for
// ilike(destinationPodLabels, '%label%'):
//   \ followed by a byte   that byte, as a literal;            \ as the last byte   a literal backslash;
//   %                      any run of bytes, the empty run included (%% is %);
//   _                      exactly one character;              every other byte     a literal.
// The pattern matches the WHOLE value (anchored at both ends), and % and _ also match a newline.  With kLikeNocase literals are folded when
// the pattern is compiled — escaped literals too — and the value's bytes when they are compared: 'A'..'Z' -> 'a'..'z' and nothing else
// (sd_fold's rule, tad_strdict.hip).
// "One character" on bytes: the byte at the position, whatever it is, and every byte in 0x80..0xBF that follows it.  On well-formed UTF-8
// that is one code point; on malformed bytes it is what it says (a run of continuation bytes at the start of a value is one character, a
// lead byte cut off at the end is one character).  The retry position behind a % advances by the same step, so a _ never starts inside
// a character.
// Two differences from the regex remain, the ones TAD_STR_CONTAINS_NOCASE has (tad.h): no Unicode case folding — 'é' does not match
// 'É' —, and Python's re.IGNORECASE lets the ASCII letters k, s and i match U+212A (Kelvin sign), U+017F (long s), U+0130 and U+0131
// (dotted capital / dotless small i), which no byte fold does.
// Plain C++ (a host program may include this header alone); no recursion, no inline assembly.
#ifndef THEIA_TAD_LIKE_H
#define THEIA_TAD_LIKE_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TAD_LIKE_FN __host__ __device__ __forceinline__
#else
#define TAD_LIKE_FN inline
#endif

namespace tad {

constexpr uint32_t kLikeMaxTokens = 1024;   // a pattern byte makes at most one token
constexpr uint32_t kLikeNocase = 1u;        // tad.h: TAD_LIKE_NOCASE (tad_internal.h asserts the two are one)

// a token: a literal is its byte (0..255); the two wildcards lie above the bytes
enum : uint16_t { kLikeOne = 0x100, kLikeAny = 0x200 };

TAD_LIKE_FN uint32_t like_fold(uint32_t c) { return c - 'A' <= (uint32_t)('Z' - 'A') ? c + 32u : c; }

// Pattern bytes -> tokens (tok has room for kLikeMaxTokens; len <= kLikeMaxTokens).  Returns the number of tokens; *min_len = the least
// number of value bytes a match needs (a literal and a _ take one byte at least, a % none).
inline uint32_t like_compile(const uint8_t *pattern, uint32_t len, uint32_t flags, uint16_t *tok, uint32_t *min_len) {
  uint32_t n = 0, need = 0;
  for (uint32_t i = 0; i < len; ++i) {
    uint32_t c = pattern[i];
    if (c == '%') {
      if (n == 0 || tok[n - 1] != kLikeAny) tok[n++] = kLikeAny;
      continue;
    }
    if (c == '_') {
      tok[n++] = kLikeOne;
      ++need;
      continue;
    }
    if (c == '\\' && i + 1 < len) c = pattern[++i];
    tok[n++] = (uint16_t)((flags & kLikeNocase) ? like_fold(c) : c);
    ++need;
  }
  if (min_len) *min_len = need;
  return n;
}

// the position behind the character that starts at i (i < len)
template <class Byte>
TAD_LIKE_FN uint32_t like_step(Byte &byte, uint32_t i, uint32_t len) {
  ++i;
  while (i < len && (byte(i) & 0xC0u) == 0x80u) ++i;
  return i;
}

// Does the program tok(0) .. tok(n - 1) match the value byte(0) .. byte(len - 1)?  tok and byte are callables (an array, LDS, words held in
// registers); byte is only ever asked for an index below len.  One backtrack point, the last % met: when the tokens behind it fail, they
// are tried again one character further on.  Worst case len * n steps.
template <class Tok, class Byte>
TAD_LIKE_FN bool like_match(Tok tok, uint32_t n, Byte &byte, uint32_t len, bool nocase) {
  uint32_t p = 0, v = 0;
  uint32_t star_p = 0, star_v = 0;      // the token behind the last %, and where in the value it is tried next
  bool star = false;
  for (;;) {
    if (p < n) {
      const uint32_t t = tok(p);
      if (t == kLikeAny) {
        if (p + 1 == n) return true;    // a trailing % takes the rest
        star = true;
        star_p = ++p;
        star_v = v;
        continue;
      }
      if (v < len) {
        if (t == kLikeOne) {
          v = like_step(byte, v, len);
          ++p;
          continue;
        }
        const uint32_t c = byte(v);
        if ((nocase ? like_fold(c) : c) == t) {
          ++v;
          ++p;
          continue;
        }
      }
    } else if (v == len) {
      return true;
    }
    if (!star || star_v >= len) return false;
    star_v = like_step(byte, star_v, len);
    v = star_v;
    p = star_p;
  }
}

}  // namespace tad

#endif  // THEIA_TAD_LIKE_H
