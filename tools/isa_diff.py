#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of two trees, kernel by kernel (CPU only; needs hipcc, no GPU).

    git worktree add /tmp/parent HEAD~1
    python tools/isa_diff.py --parent /tmp/parent train_step.hip rbf_vjp_gram.hip \\
        'irbfn::final_sum_kernel=irbfn::final_sum_kernel<float>' --diff-ok 'irbfn::mlp_head_tick_kernel'

Every unit named is compiled in both trees with the flags ``irbfn_amd.build.UNITS`` gives it (``--cuda-device-only -S``).
Comments and directives are dropped and local labels renumbered in order of appearance; kernels are paired by their
demangled name without the argument list, ``old=new`` pairs name the renamed ones.  Per kernel: SAME / DIFF, the
instruction counts, and the register / LDS / scratch / spill / occupancy figures the compiler reports.  A kernel on one
side only, or a DIFF not listed with ``--diff-ok``, makes the exit status 1."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from irbfn_amd import build as B   # noqa: E402

META = ["NumVgprs", "NumAgprs", "TotalNumSgprs", "LDSByteSize", "ScratchSize", "Occupancy"]


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    keys = []
    for d in out[:len(names)]:
        d = d[5:] if d.startswith("void ") else d
        depth, cut = 0, len(d)
        for i in range(len(d) - 1, -1, -1):                 # cut the trailing argument list "(...)"
            depth += (d[i] == ")") - (d[i] == "(")
            if depth == 0:
                cut = i
                break
        keys.append(d[:cut] if d.endswith(")") else d)
    return keys


def kernels(tree, src, extra):
    """{key: (instruction lines, {metadata})} of one compiled unit of `tree`."""
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        subprocess.run(B.compile_cmd(src, extra, ["--cuda-device-only", "-S"], f.name, root=tree), check=True)
        text = open(f.name).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    spills = {}
    for chunk in re.split(r"^  - (?=\.)", text.split("amdhsa.kernels:")[-1], flags=re.M):
        nm = re.search(r"^\s*\.name:\s*(\S+)", chunk, re.M)
        if nm:
            spills[nm.group(1).strip("'\"")] = {k: int(v) for k, v in re.findall(r"\.(sgpr_spill_count|vgpr_spill_count):\s*(\d+)", chunk)}
    res = {}
    for name, key in zip(names, demangle(names)):
        body = text.split(f"\n{name}:", 1)[1]
        body, tail = body.split(".Lfunc_end", 1)
        labels, ins = {}, []
        for ln in body.split("\n"):
            ln = ln.split(";", 1)[0].strip()
            if not ln or (ln.startswith(".") and not ln.endswith(":")):
                continue
            ins.append(re.sub(r"\.L[A-Za-z_]*\d+(?:_\d+)?", lambda m: labels.setdefault(m.group(0), f"L{len(labels)}"), ln))
        ins = [i for i in ins if not i.endswith(":") or i.startswith("L")]
        meta = {k: int(v) for k, v in re.findall(r"^; (\w+): (\d+)\b", tail.split(".amdhsa_kernel", 1)[0], re.M) if k in META}
        meta.update(spills.get(name, {}))
        res[key if key not in res else key + "#" + name] = (ins, meta)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True, help="checkout of the parent commit")
    ap.add_argument("--new", default=HERE)
    ap.add_argument("--diff-ok", action="append", default=[], help="kernel (new name) whose DIFF is expected")
    ap.add_argument("items", nargs="+", help="unit sources (x.hip) and old=new kernel renames")
    a = ap.parse_args()
    ren = dict(i.split("=", 1) for i in a.items if "=" in i)
    bad = 0
    for src in [i for i in a.items if "=" not in i]:
        for s, obj, extra in [u for u in B.UNITS if u[0] == src]:
            old, new = kernels(a.parent, s, extra), kernels(a.new, s, extra)
            print(f"== {s} {' '.join(extra)} ({obj}): {len(old)} kernels in the parent, {len(new)} now")
            seen = set()
            for k, (oi, om) in old.items():
                nk = ren.get(k, k)
                if nk not in new:
                    print(f"ONLY IN PARENT  {k}")
                    bad += 1
                    continue
                seen.add(nk)
                ni, nm = new[nk]
                same = oi == ni
                bad += (not same) and nk not in a.diff_ok
                fmt = lambda m: " ".join(f"{x}={m.get(x, '?')}" for x in META + ["sgpr_spill_count", "vgpr_spill_count"])
                print(f"{'SAME' if same else 'DIFF'}  {k}{'' if nk == k else ' -> ' + nk}  instructions {len(oi)} -> {len(ni)}")
                print(f"      {fmt(om)}" if om == nm else f"      parent: {fmt(om)}\n      new:    {fmt(nm)}")
            for k in new.keys() - seen:
                print(f"ONLY IN NEW     {k}")
                bad += 1
    print("RESULT:", "ok" if not bad else f"{bad} unlisted DIFF / unpaired kernel(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
