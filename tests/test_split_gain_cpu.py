"""The two forms of K1g's operand split (split_pair_mix, irbfn_amd/csrc/rbf_forward_gram.h) restated on the host and compared
bit for bit: the 2^11 gain of the lo half as two multiplies in front of the mixes (the form before), and as ONE 64-bit integer add
on the pair of residuals behind them (11 added to both exponent fields).  A stand-alone C++17 program, built with the host compiler
and run, as tests/test_dispatch_cpu.py does; the packed round-toward-zero conversion to f16 is emulated on the bits, the mixes
are fmaf (correctly rounded, no contraction).

The sweep: every exponent field from 0 (zero and the subnormals) to 2^14 -- the largest P = 2^14 phi -- of both signs with
mantissas 0, all ones, single bits and 2000 pseudo-random ones, the second value of the pair drawn independently (any exponent,
any sign); +-0, the largest subnormal, the smallest normal and 2^14 exactly by name.  Across it (hi, lo) must be identical, and
the add must not carry out of the low dword (asserted on the operand of the add).  It also says why the add sits BEHIND the
mixes: added to P in front of them (in place, P being dead behind the hi conversion) the same five instructions give the same
pair everywhere except at P = -0, whose lo becomes -0 where the multiplies give +0."""
import subprocess

from test_dispatch_cpu import _host_compiler

import pytest

PROGRAM = r"""
#include <assert.h>
#include <initializer_list>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float flt(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// v_cvt_pkrtz_f16_f32 on one value: round toward zero, subnormal results kept, the sign kept on a zero (finite inputs below 2^16)
static uint16_t rtz16(float f) {
  const uint32_t u = bits(f), s = (u >> 16) & 0x8000u, e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
  if (e == 0) return (uint16_t)s;                            // f32 zero or subnormal: below every f16 subnormal
  const int E = (int)e - 127;
  assert(E < 16);
  if (E >= -14) return (uint16_t)(s | (uint32_t)(E + 15) << 10 | m >> 13);
  const int sh = 13 + (-14 - E);                             // f16 subnormal: the 24-bit significand moved down
  return (uint16_t)(s | (sh > 24 ? 0u : (m | 0x800000u) >> sh));
}
static float f16_to_f32(uint16_t h) {                        // exact
  const int e = (h >> 10) & 31, m = h & 1023;
  const float v = e == 0 ? ldexpf((float)m, -24) : ldexpf((float)(m | 1024), e - 25);
  return (h & 0x8000) ? -v : v;
}

struct Pair { uint32_t hi, lo; };
static const uint64_t kGain2 = 0x0580000005800000ull;        // 11 << 23 in both dwords

static Pair split_mul(float p0, float p1) {                  // the form before: q = 2048 P, lo = rtz(fma(hi, -2048, q))
  const uint16_t h0 = rtz16(p0), h1 = rtz16(p1);
  const float q0 = p0 * 2048.0f, q1 = p1 * 2048.0f;
  const float d0 = fmaf(f16_to_f32(h0), -2048.0f, q0), d1 = fmaf(f16_to_f32(h1), -2048.0f, q1);
  return Pair{(uint32_t)h0 | (uint32_t)h1 << 16, (uint32_t)rtz16(d0) | (uint32_t)rtz16(d1) << 16};
}
static Pair split_add(float p0, float p1) {                  // d = fma(hi, -1, P), one 64-bit add on (d0, d1), lo = rtz
  const uint16_t h0 = rtz16(p0), h1 = rtz16(p1);
  const float d0 = fmaf(f16_to_f32(h0), -1.0f, p0), d1 = fmaf(f16_to_f32(h1), -1.0f, p1);
  assert((uint64_t)bits(d0) + 0x05800000u <= 0xffffffffull);             // no carry out of the low dword
  const uint64_t dd = ((uint64_t)bits(d0) | (uint64_t)bits(d1) << 32) + kGain2;
  return Pair{(uint32_t)h0 | (uint32_t)h1 << 16, (uint32_t)rtz16(flt((uint32_t)dd)) | (uint32_t)rtz16(flt((uint32_t)(dd >> 32))) << 16};
}
static Pair split_add_in_front(float p0, float p1) {         // the add on (P0, P1) in front of the mixes: lo = rtz(fma(hi, -2048, q))
  const uint16_t h0 = rtz16(p0), h1 = rtz16(p1);
  assert((uint64_t)bits(p0) + 0x05800000u <= 0xffffffffull);
  const uint64_t qq = ((uint64_t)bits(p0) | (uint64_t)bits(p1) << 32) + kGain2;
  const float d0 = fmaf(f16_to_f32(h0), -2048.0f, flt((uint32_t)qq)), d1 = fmaf(f16_to_f32(h1), -2048.0f, flt((uint32_t)(qq >> 32)));
  return Pair{(uint32_t)h0 | (uint32_t)h1 << 16, (uint32_t)rtz16(d0) | (uint32_t)rtz16(d1) << 16};
}

static long npairs = 0, nonzero_lo = 0, front_differs = 0;
static void check(uint32_t b0, uint32_t b1) {
  const float p0 = flt(b0), p1 = flt(b1);
  const Pair a = split_mul(p0, p1), b = split_add(p0, p1), c = split_add_in_front(p0, p1);
  if (a.hi != b.hi || a.lo != b.lo) {
    printf("MISMATCH p = %08x %08x: hi %08x / %08x lo %08x / %08x\n", b0, b1, a.hi, b.hi, a.lo, b.lo);
    assert(0);
  }
  // in front of the mixes: the same pair unless one of the two values is -0, whose half of lo is then -0 for +0
  const uint32_t want = a.lo | (b0 == 0x80000000u ? 0x8000u : 0u) | (b1 == 0x80000000u ? 0x80000000u : 0u);
  assert(c.hi == a.hi && c.lo == want);
  front_differs += c.lo != a.lo;
  ++npairs;
  nonzero_lo += (a.lo & 0x7fff7fffu) != 0;
}

int main() {
  assert(rtz16(1.0f) == 0x3c00 && rtz16(-2.0f) == 0xc000 && rtz16(65504.0f) == 0x7bff && rtz16(16384.0f) == 0x7400);
  assert(rtz16(ldexpf(1.0f, -24)) == 1 && rtz16(ldexpf(1.9999f, -25)) == 0 && rtz16(-ldexpf(1.0f, -30)) == 0x8000 && rtz16(-0.0f) == 0x8000);
  assert(rtz16(1.9999f) == 0x3fff);                         // truncated, not rounded up to 2
  assert(f16_to_f32(0x3c00) == 1.0f && f16_to_f32(0x0001) == ldexpf(1.0f, -24) && f16_to_f32(0xfbff) == -65504.0f);
  const uint32_t P14 = 0x46800000u;                          // 2^14
  assert(flt(P14) == 16384.0f);
  uint32_t rnd = 12345u;
  auto next = [&]() { rnd = rnd * 1664525u + 1013904223u; return rnd; };
  auto any = [&]() {                                         // any value of the domain: exponent field <= 2^14's, either sign
    const uint32_t r = next(), e = (next() >> 8) % 142u;
    return (r & 0x80000000u) | e << 23 | (e == 141u ? 0u : (next() >> 9));
  };
  for (uint32_t e = 0; e <= 141u; ++e)
    for (uint32_t s = 0; s < 2; ++s) {
      const uint32_t base = s << 31 | e << 23;
      if (e == 141u) { check(base, any()); check(any(), base); check(base, base); continue; }   // 2^14 exactly, of either sign
      for (uint32_t m : {0u, 0x7fffffu, 1u, 0x400000u, 0x001000u, 0x000fffu, 0x7ff000u, 0x002000u, 0x001fffu}) {
        check(base | m, any());
        check(any(), base | m);
        check(base | m, base | (m ^ 0x155555u));
      }
      for (int k = 0; k < 2000; ++k) {
        const uint32_t m = next() >> 9;
        check(base | m, any());
        check(any(), base | (next() >> 9));
      }
    }
  // by name: +-0, the largest subnormal, the smallest normal, 2^14
  const uint32_t named[] = {0x00000000u, 0x80000000u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u, P14, P14 | 0x80000000u};
  for (uint32_t a : named)
    for (uint32_t b : named) check(a, b);
  {
    const Pair z = split_add(-0.0f, 0.0f);                   // hi keeps the sign of the zero, lo is +0 in both halves
    assert(z.hi == 0x00008000u && z.lo == 0u);
    const Pair t = split_add(16384.0f, -16384.0f);
    assert(t.hi == 0xf4007400u && t.lo == 0u);
    const Pair u = split_add(1.0f + ldexpf(1.0f, -11), ldexpf(1.0f, -20) * (1.0f + ldexpf(1.0f, -23)));
    assert(u.hi == (0x3c00u | (uint32_t)rtz16(ldexpf(1.0f, -20)) << 16) && (u.lo & 0xffffu) == 0x3c00u);   // lo = 2^11 x 2^-11 = 1
    assert((u.lo >> 16) == rtz16(ldexpf(1.0f, -32)));       // 2^11 x 2^-43: below the f16 subnormals
  }
  assert(npairs > 1000000 && nonzero_lo > npairs / 4 && front_differs > 0);
  printf("split ok %ld pairs\n", npairs);
  return 0;
}
"""


def test_split_gain_standalone(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "split_gain_test.cpp", tmp_path / "split_gain_test"
    src.write_text(PROGRAM)
    # no -DNDEBUG: the asserts are the test; no contraction: every product and sum is rounded as written
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", str(src), "-o", str(exe), "-lm"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().startswith("split ok")
