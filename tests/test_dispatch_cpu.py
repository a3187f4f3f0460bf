"""irbfn::dispatch (irbfn_amd/csrc/dispatch.h) on its own: the run-time value -> compile-time constant step every
launcher goes through, compiled into a stand-alone C++17 program with the host compiler and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <assert.h>
#include <stdio.h>
#include <initializer_list>
#include "dispatch.h"
using irbfn::dispatch;

int main() {
  // a value on the list: f runs exactly once, with the constant equal to the value; its status comes back unchanged
  for (int status : {0, 7, -3, (int)IRBFN_ERR_UNSUPPORTED}) {
    for (int v : {3, 4, 7, 8}) {
      int calls = 0, seen = -1;
      const int rc = dispatch<3, 4, 7, 8>(v, [&](auto c) {
        static_assert(decltype(c)::value == c(), "a compile-time constant");
        ++calls; seen = c();
        return status;
      });
      assert(calls == 1 && seen == v && rc == status);
    }
  }
  // a value off the list: nothing runs
  for (int v : {-1, 0, 5, 6, 9, 1 << 30}) {
    int calls = 0;
    const int rc = dispatch<3, 4, 7, 8>(v, [&](auto) { ++calls; return 0; });
    assert(rc == IRBFN_ERR_UNSUPPORTED && calls == 0);
  }
  // nested lists reach the one matching (a, b, c); one value off its list reaches none
  for (int a = 0; a < 10; ++a)
    for (int b = 0; b < 4; ++b)
      for (int c = 0; c < 20; ++c) {
        int calls = 0, got = 0;
        const int rc = dispatch<3, 4, 7, 8>(a, [&](auto ca) {
          return dispatch<0, 1, 2>(b, [&](auto cb) {
            return dispatch<2, 5, 10, 16>(c, [&](auto cc) {
              constexpr int key = ca() * 10000 + cb() * 100 + cc();   // usable as a template argument
              ++calls; got = key;
              return 1;
            });
          });
        });
        const bool on = (a == 3 || a == 4 || a == 7 || a == 8) && b < 3 && (c == 2 || c == 5 || c == 10 || c == 16);
        if (on) assert(rc == 1 && calls == 1 && got == a * 10000 + b * 100 + c);
        else assert(rc == IRBFN_ERR_UNSUPPORTED && calls == 0);
      }
  puts("dispatch ok");
  return 0;
}
"""


def _host_compiler():
    rocm = [os.path.join(os.path.dirname(os.path.dirname(h)), "llvm", "bin", "clang++")
            for h in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if h]
    for cand in [shutil.which("g++"), shutil.which("clang++"), *rocm]:
        if cand and os.path.exists(cand):
            return cand
    return None


def test_dispatch_standalone(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "dispatch_test.cpp", tmp_path / "dispatch_test"
    src.write_text(PROGRAM)
    # no -DNDEBUG: the asserts are the test
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "irbfn_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "dispatch ok"
